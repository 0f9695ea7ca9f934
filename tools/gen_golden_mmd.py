"""Writes tests/golden/mmd.pt: what the reference's mmd.py gives on the case table of tests/ref_mmd.py.  Needs scipy (the
reference's cdist); the tests do not: they read the golden.

    python tools/gen_golden_mmd.py <reference checkout>/packages/viscy-utils/src/viscy_utils/evaluation/mmd.py

The reference module is loaded by path.  Inputs are not stored: the table rebuilds them from seeds.  Per case:
  bandwidth     the reference's median_heuristic(X, Y)
  mmd2, p_value, null   the reference's mmd_permutation_test with that bandwidth passed explicitly (null float32, as returned)
  err_ref       max |reference - float64 restatement| over mmd2 and the null
  gap           min |null - observed| of the restatement: asserted >= 100 err_ref, so the p-value can be compared for equality
  dist_err_f32  max |D - D64| of the float32 numpy emulation of the centred Gram form on the median heuristic's rows
LABEL_CASES also carry the reference's label matrix (z_obs over z_null, captured from its own run), KERNEL_CASES its
gaussian_rbf_kernel(X, Y, bandwidth) and the emulation's maximum error of the exponent."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_mmd as RM  # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_mmd", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_labels(ref, X, Y, P, seed):
    """the label matrices the reference multiplies its kernel by, captured from one run.  _mmd2_from_labels forms three products
    per call (K @ z.T, K @ (1 - z).T twice), first for z_obs, then for z_null: right operands 0 and 3 are the two matrices"""
    calls = []

    class Spy(np.ndarray):
        def __matmul__(self, other):
            calls.append(np.asarray(other).T.copy())
            return np.asarray(self) @ np.asarray(other)

    real = ref.gaussian_rbf_kernel
    ref.gaussian_rbf_kernel = lambda a, b, bw: real(a, b, bw).view(Spy)
    try:
        ref.mmd_permutation_test(X, Y, n_permutations=P, bandwidth=1.0, seed=seed)
    finally:
        ref.gaussian_rbf_kernel = real
    assert len(calls) == 6 and calls[0].shape == (1, len(X) + len(Y)) and calls[3].shape == (P, len(X) + len(Y))
    assert (calls[0] + calls[1] == 1).all() and (calls[3] + calls[4] == 1).all()
    return np.concatenate([calls[0], calls[3]], axis=0).astype(np.uint8)


def main():
    import scipy

    ref = load_reference(sys.argv[1])
    out = {"cases": {}, "numpy": np.__version__, "scipy": scipy.__version__}
    for name, c in RM.CASES.items():
        X, Y = RM.build(name)
        bw = ref.median_heuristic(X, Y)
        obs, p, null = ref.mmd_permutation_test(X, Y, n_permutations=c["P"], bandwidth=bw, seed=c["pseed"])
        ours = RM.restatement(name, bw)
        err_ref = float(max(abs(obs - ours[0]), np.abs(null.astype(np.float64) - ours[1:]).max()))
        gap = float(np.abs(ours[1:] - ours[0]).min())
        p_ours = float((np.sum(ours[1:] >= ours[0]) + 1) / (c["P"] + 1))
        entry = {"bandwidth": float(bw), "mmd2": float(obs), "p_value": float(p), "null": torch.from_numpy(np.asarray(null).copy()),
                 "err_ref": err_ref, "gap": gap, "dist_err_f32": RM.dist_err_f32(X, Y)}
        print(f"{name:28s} bw {bw:10.4f}  mmd2 {obs: .6e}  p {p:.4f}  err_ref {err_ref:.2e}  gap {gap:.2e}  dist_err_f32 {entry['dist_err_f32']:.2e}")
        assert gap >= 100 * err_ref, (name, gap, err_ref)
        assert p_ours == p, (name, p_ours, p)
        if name in RM.LABEL_CASES:
            z = reference_labels(ref, X, Y, c["P"], c["pseed"])
            assert z.shape == (c["P"] + 1, c["n"] + c["m"])
            entry["labels"] = torch.from_numpy(z)
        if name in RM.KERNEL_CASES:
            entry["kernel"] = torch.from_numpy(ref.gaussian_rbf_kernel(X, Y, bw).copy())
            entry["exponent_err_f32"] = RM.exponent_err_f32(X, Y, bw)
            print(f"{'':28s} kernel {tuple(entry['kernel'].shape)}  exponent_err_f32 {entry['exponent_err_f32']:.2e}")
        out["cases"][name] = entry
    path = os.path.join(ROOT, "tests", "golden", "mmd.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
