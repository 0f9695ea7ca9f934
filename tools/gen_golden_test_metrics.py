"""Writes tests/golden/test_metrics.pt: what the reference's own ``ssim_25d`` / ``ms_ssim_25d`` return on the CPU for the seeded
stacks of tests/ref_test_metrics.py (``GOLDEN_CASES``, rebuilt from the seed by the tests).

    python tools/gen_golden_test_metrics.py <checkout of the reference>/packages/viscy-utils/src/viscy_utils/evaluation/metrics.py

The reference module is loaded by path.  Its two functions need torch alone; the module's top-level imports of packages that are not
installed (segmentation metrics: scikit-image, torchmetrics' detection module, torchvision) are satisfied by empty stand-ins.
Results only: per case and per call of ``ref_test_metrics.golden_calls`` the returned tensors, in fp32 as the reference returns them."""
import importlib
import importlib.util
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_test_metrics as R  # noqa: E402

_NEEDS = {"scipy.optimize": ("linear_sum_assignment",), "skimage.measure": ("label", "regionprops"),
          "torchmetrics.detection.mean_ap": ("MeanAveragePrecision",), "torchvision.ops": ("masks_to_boxes",)}


def load_reference(path):
    for name, attrs in _NEEDS.items():
        try:
            importlib.import_module(name)
            continue
        except Exception:  # noqa: BLE001 - absent or unusable here: none of it is called
            pass
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
        for a in attrs:
            setattr(sys.modules[name], a, None)
    spec = importlib.util.spec_from_file_location("reference_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    out = {"cases": {}, "torch": str(torch.__version__)}
    for name, case in R.GOLDEN_CASES.items():
        pred, target = R.golden_stacks(name)
        rec = {"shape": tuple(case["shape"]), "seed": case["seed"]}
        for key, fn, kw in R.golden_calls(name):
            with torch.no_grad():
                res = getattr(ref, fn)(pred, target, **kw)
            rec[key] = tuple(r.clone() for r in res) if isinstance(res, tuple) else res.clone()
            print(name, key, [r.tolist() for r in res] if isinstance(res, tuple) else res.tolist())
        out["cases"][name] = rec
    path = os.path.join(ROOT, "tests", "golden", R.GOLDEN_FILE)
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
