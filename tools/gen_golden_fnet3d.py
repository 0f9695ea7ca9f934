"""Writes tests/golden/fnet3d.pt from the reference's own FNet3D (viscy_models/unet/{blocks.py, unet3d_base.py, unet3d.py}, loaded
by path under stub ``viscy_models`` / ``viscy_models.unet`` packages; they are torch-only).

Per case (small depth / width, B = 2, Z != Y != X): the constructor kwargs, the state dict, the input, the training-mode output,
the loss <out, gout> under a fixed upstream gradient ``gout`` and every parameter gradient, the running statistics after that one
step and the eval-mode output that uses them.  Plus the state-dict key list, shapes and parameter count of the full depth-3 and
depth-4 (mult_chan 32) models.  The file holds tensors, dicts, lists and numbers only.

    python tools/gen_golden_fnet3d.py --ref <reference checkout> [--out tests/golden/fnet3d.pt]
"""

from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = os.path.join("packages", "viscy-models", "src", "viscy_models", "unet")

CASES = [
    ("d2_m4_out1", dict(in_channels=1, out_channels=1, depth=2, mult_chan=4), (2, 1, 8, 16, 24)),
    ("d3_m2_out2", dict(in_channels=1, out_channels=2, depth=3, mult_chan=2), (2, 1, 8, 16, 24)),
]


def load_reference(ref_root: str):
    d = os.path.join(ref_root, SUB)
    for name in ("viscy_models", "viscy_models.unet"):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = []
            sys.modules[name] = pkg
    for mod in ("blocks", "unet3d_base", "unet3d"):
        name = f"viscy_models.unet.{mod}"
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, mod + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
    return sys.modules["viscy_models.unet.unet3d"].Unet3d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fnet3d.pt"))
    a = ap.parse_args()
    torch.set_num_threads(8)
    Unet3d = load_reference(a.ref)
    golden = {"cases": {}, "full": {}}
    for depth in (3, 4):
        net = Unet3d(in_channels=1, out_channels=1, depth=depth, mult_chan=32)
        sd = net.state_dict()
        golden["full"][depth] = dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()],
                                     numel=sum(p.numel() for p in net.parameters()))
    for i, (name, kw, shape) in enumerate(CASES):
        torch.manual_seed(100 + i)
        net = Unet3d(**kw).train()
        sd0 = {k: v.clone() for k, v in net.state_dict().items()}
        g = torch.Generator().manual_seed(200 + i)
        x = torch.randn(shape, generator=g)
        out = net(x)
        gout = torch.randn(out.shape, generator=g)
        loss = (out * gout).sum()
        loss.backward()
        grads = {k: p.grad.clone() for k, p in net.named_parameters()}
        after = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
        net.eval()
        with torch.no_grad():
            out_eval = net(x)
        golden["cases"][name] = dict(kwargs=kw, state_dict=sd0, x=x, out=out.detach(), gout=gout, loss=loss.detach(), grads=grads,
                                     buffers_after=after, out_eval=out_eval)
        print(name, tuple(out.shape), float(loss.detach()))
    torch.save(golden, a.out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
