"""The DynaCLR patch feed, event-timed on the device: viscy_amd.ops.patch_gather (vsx_patch_gather: one launch per batch, the
descriptor table built and uploaded inside the call) against plain torch on the same resident frames,
    torch.stack([f[:, :, y0:y1, x0:x1] for ...]).float()
and next to a Tensor.copy_ of the same byte count.  Writes profiles/triplet_feed_perf.txt (OUT=... elsewhere).

Shapes.  Both are read off the comments of the DynaCLR recipes, they are NOT measured workloads:
  predict   2 channels, Z = 1, 160 x 160 patches, B = 32, float32 frames of 2048 x 2048 (8 cells per frame)
  fit 3-D   2 channels, Z = 30, 384 x 384 patches, 64 triplets = 192 patches, uint16 frames of 2048 x 2048 (12 patches per frame)
Method: every form is warmed up, then timed in WINDOWS of REPS calls between two device events; the forms alternate window by
window in the same process and the median window is reported, with the spread (min .. max).  Bytes = what the gather must move:
n C Z Yp Xp (source element size + 4).  Last: one predict epoch of TripletDataModule over a synthetic plate written to a temporary
directory, device cut (cold cache, then warm) against the host cut plus one upload per batch, host clock around a synchronise.
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viscy_amd import _lib, ops  # noqa: E402

assert torch.cuda.is_available(), "perf_triplet_feed measures on the MI355X: no device, no number"
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "triplet_feed_perf.txt"))
WINDOWS = int(os.environ.get("WINDOWS", 7))
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(forms: dict, reps: int) -> dict:
    """{name: (median, min, max) ms per call}: warm-up of every form, then WINDOWS rounds visiting the forms in turn"""
    for fn in forms.values():
        window(fn, max(2, reps // 4))
    t = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            t[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def gather_shape(tag, dtype, n_frames, C, Z, HW, n, P, reps):
    g = torch.Generator(device="cuda").manual_seed(n)
    if dtype == torch.float32:
        frames = [torch.randn(C, Z, HW, HW, device="cuda", generator=g) for _ in range(n_frames)]
    else:
        frames = [torch.randint(-32768, 32768, (C, Z, HW, HW), device="cuda", generator=g, dtype=torch.int16).view(dtype) for _ in range(n_frames)]
    rng = np.random.default_rng(n)
    src = [frames[i * n_frames // n] for i in range(n)]   # cells of one frame are neighbours in the batch, as in predict
    org = [(int(rng.integers(0, HW - P + 1)), int(rng.integers(0, HW - P + 1))) for _ in range(n)]
    esize = frames[0].element_size()
    moved = n * C * Z * P * P * (esize + 4)
    out = torch.empty((n, C, Z, P, P), device="cuda")
    table = ops.patch_descriptors(src, org, (P, P)).to("cuda")
    code = ops.PATCH_GATHER_DTYPES[dtype]

    def wrapper():
        return ops.patch_gather(src, org, (P, P), out=out)

    def kernel_only():
        _lib.check(_lib.lib().vsx_patch_gather(_lib.ptr(table), _lib.ptr(out), n, C, Z, P, P, code, _lib.stream()), "patch_gather")

    def torch_form():
        return torch.stack([f[:, :, y0 : y0 + P, x0 : x0 + P] for f, (y0, x0) in zip(src, org)]).float()

    form = "torch.stack of slices, .float()"
    try:
        torch_form()
    except (RuntimeError, NotImplementedError):   # no uint16 stack on this torch: the same bytes through the int16 view
        def torch_form():  # noqa: F811
            return torch.stack([f.view(torch.int16)[:, :, y0 : y0 + P, x0 : x0 + P] for f, (y0, x0) in zip(src, org)]).view(dtype).float()

        form = "torch.stack of int16-viewed slices, .view(uint16).float()"

    a = torch.empty(moved // 8, device="cuda")   # copy_ reads and writes 4 bytes per element: the same bytes in all
    b = torch.empty_like(a)
    same = torch.equal(wrapper().view(torch.int32), torch_form().view(torch.int32))
    r = alternate({"patch_gather": wrapper, "kernel": kernel_only, "torch": torch_form, "copy_": lambda: b.copy_(a)}, reps)
    say(f"{tag}: n = {n} patches of ({C}, {Z}, {P}, {P}) from {n_frames} {str(dtype).replace('torch.', '')} frames ({C}, {Z}, {HW}, {HW}); "
        f"{moved / 2 ** 20:.1f} MiB moved; bits equal to the torch form: {same}; windows of {reps} calls, {WINDOWS} windows per form")
    for k in ("patch_gather", "kernel", "torch", "copy_"):
        med, lo, hi = r[k]
        what = {"patch_gather": "ops.patch_gather (table build + upload + launch)", "kernel": "vsx_patch_gather alone (table resident)",
                "torch": form, "copy_": "Tensor.copy_ of the same byte count"}[k]
        say(f"  {what:58s} {med * 1e3:10.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})   {moved / med / 1e9:8.3f} TB/s")
    say(f"  torch / ops.patch_gather = {r['torch'][0] / r['patch_gather'][0]:.2f}x   (the bar: >= 1)")
    del frames, src, out, a, b
    torch.cuda.empty_cache()


def predict_epoch():
    import pandas as pd

    from viscy_amd.data import write_hcs_plate
    from viscy_amd.data.triplet import TripletDataModule

    fovs, T, HW, cells, P, B = ["A/1/0", "A/1/1"], 4, 2048, 64, 160, 32
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        arrays = {f: rng.random((T, 2, 1, HW, HW), dtype=np.float32) for f in fovs}
        write_hcs_plate(os.path.join(d, "p.zarr"), arrays, ["Phase", "Fluor"])
        for f in fovs:
            rows = [{"track_id": k, "t": t, "id": k * T + t, "parent_track_id": -1, "parent_id": -1, "z": 0,
                     "y": int(rng.integers(P // 2 + 1, HW - P // 2)), "x": int(rng.integers(P // 2 + 1, HW - P // 2))}
                    for t in range(T) for k in range(cells)]
            os.makedirs(os.path.join(d, "tracks", f))
            pd.DataFrame(rows).sort_values(["t", "track_id"]).to_csv(os.path.join(d, "tracks", f, "t.csv"), index=False)

        def epoch(dm, upload):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for batch in dm.predict_dataloader():
                x = batch["anchor"].to("cuda", non_blocking=True) if upload else batch["anchor"]
                n += x.shape[0]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, n

        def module(device):
            dm = TripletDataModule(os.path.join(d, "p.zarr"), os.path.join(d, "tracks"), ["Phase", "Fluor"], (0, 1), (P, P), (P, P),
                                   batch_size=B)
            dm.device = device
            dm.setup("predict")
            return dm

        epoch(module("cuda"), False)   # warm-up: code objects, allocator, page cache of the store
        res = {}
        for _ in range(3):             # alternating, a fresh (cold) cache for every device epoch
            dev = module("cuda")
            res.setdefault("device, cold cache", []).append(epoch(dev, False)[0])
            res.setdefault("device, warm cache", []).append(epoch(dev, False)[0])
            host = module("cpu")
            ms, n = epoch(host, True)
            res.setdefault("host cut + upload", []).append(ms)
        say(f"predict epoch: {len(fovs)} FOVs x {T} time points of (2, 1, {HW}, {HW}) float32, {n} cells, patches {P} x {P}, B = {B}; "
            "host clock around a synchronise, 3 alternating rounds, median (min .. max)")
        for k, v in res.items():
            say(f"  {k:24s} {statistics.median(v):9.1f} ms  ({min(v):.1f} .. {max(v):.1f})")


say(f"# tools/perf_triplet_feed.py on {torch.cuda.get_device_name(0)}; the shapes come from the recipes' comments, they are not measured workloads")
gather_shape("predict", torch.float32, 4, 2, 1, 2048, 32, 160, reps=200)
gather_shape("fit 3-D", torch.uint16, 16, 2, 30, 2048, 192, 384, reps=5)
predict_epoch()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
