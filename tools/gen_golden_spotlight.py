"""Writes tests/golden/spotlight.pt: what the reference's SpotlightLoss gives on the case table of tests/ref_spotlight.py.

    python tools/gen_golden_spotlight.py <checkout of the reference>/packages/viscy-utils/src/viscy_utils/losses/spotlight.py

The reference module is loaded by path (it needs torch alone).  Inputs are not stored: the table rebuilds them from seeds and
shapes.  Per case: the shape, the reference's loss in fp32 and in float64, and its gradient (times gout) in both precisions at
``ref_spotlight.grad_sample_index`` (every entry for small cases).  Per threshold case: the reference's Otsu thresholds."""
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_spotlight as RS  # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_spotlight", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, inp, dtype):
    fn = ref.SpotlightLoss(fg_threshold=inp["fg_threshold"])
    p = inp["pred"].to(dtype).detach().clone().requires_grad_(True)
    loss = fn(p, inp["target"].to(dtype), fg_mask=inp["fg_mask"])
    (loss * inp["gout"]).backward()
    return loss.detach(), p.grad.reshape(-1)


def main():
    ref = load_reference(sys.argv[1])
    out = {"cases": {}, "otsu": {}, "torch": str(torch.__version__)}
    for name, case in RS.CASES.items():
        inp = RS.build(name)
        idx = RS.grad_sample_index(inp["pred"].numel())
        l32, g32 = run(ref, inp, torch.float32)
        l64, g64 = run(ref, inp, torch.float64)
        out["cases"][name] = {"shape": tuple(case["shape"]), "loss32": l32.clone(), "loss64": l64.clone(),
                              "grad32": g32[idx].clone(), "grad64": g64[idx].clone()}
        print(f"{name:18s} loss {l32.item():.7f}  |fp32 - fp64| / |fp64| = {abs(l32.item() - l64.item()) / abs(l64.item()):.2e}")
    for name in RS.OTSU_CASES:
        t = RS.otsu_target(name)
        thr = ref._otsu_threshold_batch(t).reshape(t.shape[0], t.shape[1]).clone()
        out["otsu"][name] = {"shape": tuple(t.shape), "thr": thr}
        print(f"otsu {name}: {thr.flatten().tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "spotlight.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
