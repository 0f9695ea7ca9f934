"""The multi-experiment DynaCLR feed, timed on the device at the DynaCLR-3D-BagOfChannels-v2 shape (z_extraction_window 45,
yx_patch_size 256 x 256, batch_size 256, one channel per sample).  Writes profiles/multi_experiment_feed.txt (OUT=... elsewhere).

  1. identity   vsx_patch_gather_scaled with arange tables against vsx_patch_gather on the same boxes (tables resident, kernels
                alone).  The bar: not slower by more than the run-to-run spread this session shows for either kernel.
  2. two scales the same launch over a mixed batch, half the patches upsampled from (34, 192, 192) boxes (scale 0.75), half
                downsampled from (68, 384, 384) boxes (scale 1.5), as bytes written per second against the identity case.
  3. a batch    one ``MultiExperimentTripletDataset.__getitems__`` call (256 anchors and their positives, warm frame cache) against
                the reference's procedure restated on the host over frames already in memory: numpy cut, CPU
                ``F.interpolate(mode="nearest-exact")`` per patch, ``torch.stack``, ``.to(device)``.

Method: every form is warmed up, then timed in WINDOWS of REPS calls between two device events (3: a host clock around a
synchronise); forms alternate window by window in one process; the median window is reported with the spread (min .. max).
``--rehearse`` builds the stores, the table and one host-path batch at a small size and stops before anything is timed.
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REHEARSE = "--rehearse" in sys.argv
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "multi_experiment_feed.txt"))
WINDOWS = int(os.environ.get("WINDOWS", 7))
ZT, PATCH, BATCH = (6, 32, 16) if REHEARSE else (45, 256, 256)   # the recipe's z_extraction_window, yx_patch_size, batch_size
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


def row(name, stat, written):
    med, lo, hi = stat
    say(f"  {name:<58s} {med * 1e3:9.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})   {written / med / 1e9:7.3f} TB/s written")


# ------------------------------------------------------------------------------------------------ 1 and 2: the kernels
def kernels():
    from viscy_amd import _lib, ops
    from viscy_amd.data import nearest_exact_index

    n, HW, Zf = BATCH, 1024, 72
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = [torch.randn(1, Zf, HW, HW, device="cuda", generator=g) for _ in range(8)]
    rng = np.random.default_rng(1)
    src = [frames[i * len(frames) // n] for i in range(n)]
    written = n * ZT * PATCH * PATCH * 4
    out = torch.empty((n, 1, ZT, PATCH, PATCH), device="cuda")
    out2 = torch.empty_like(out)

    def upload(desc, idx):
        words = desc.numel()
        both = torch.empty(words + (idx.numel() + 1) // 2, dtype=torch.int64)
        both[:words] = desc.reshape(-1)
        both[words:].view(torch.int32)[: idx.numel()] = idx
        dev = both.cuda()
        return dev, dev[words:]

    # identity: the same (y0, x0) boxes, Z planes [10, 10 + ZT) of every frame
    org = [(int(rng.integers(0, HW - PATCH + 1)), int(rng.integers(0, HW - PATCH + 1))) for _ in range(n)]
    views = {id(f): f[:, 10 : 10 + ZT] for f in frames}
    plain_src = [views[id(f)] for f in src]
    table = ops.patch_descriptors(plain_src, org, (PATCH, PATCH)).cuda()
    chan, zs = np.arange(1), 10 + np.arange(ZT)
    desc, idx, shape = ops.patch_tables(src, [chan] * n, [zs] * n, [y0 + np.arange(PATCH) for y0, _ in org],
                                        [x0 + np.arange(PATCH) for _, x0 in org])
    assert shape == tuple(out.shape)
    d_id, i_id = upload(desc, idx)
    code = ops.PATCH_GATHER_DTYPES[torch.float32]

    def plain():
        _lib.check(_lib.lib().vsx_patch_gather(_lib.ptr(table), _lib.ptr(out2), n, 1, ZT, PATCH, PATCH, code, _lib.stream()), "patch_gather")

    def scaled(d, i):
        def call():
            _lib.check(_lib.lib().vsx_patch_gather_scaled(_lib.ptr(d), _lib.ptr(i), _lib.ptr(out), n, 1, ZT, PATCH, PATCH, code,
                                                          _lib.stream()), "patch_gather_scaled")
        return call

    # two scales: boxes of (34, 192, 192) and (68, 384, 384) resampled to (ZT, PATCH, PATCH)
    chans, tz, ty, tx = [], [], [], []
    for p in range(n):
        nz, nyx = ((ZT * 3 + 2) // 4, PATCH * 3 // 4) if p % 2 == 0 else (min(ZT * 3 // 2, Zf), PATCH * 3 // 2)
        z0, y0, x0 = int(rng.integers(0, Zf - nz + 1)), int(rng.integers(0, HW - nyx + 1)), int(rng.integers(0, HW - nyx + 1))
        chans.append(chan)
        tz.append(z0 + nearest_exact_index(nz, ZT))
        ty.append(y0 + nearest_exact_index(nyx, PATCH))
        tx.append(x0 + nearest_exact_index(nyx, PATCH))
    desc, idx, _ = ops.patch_tables(src, chans, tz, ty, tx)
    d_mix, i_mix = upload(desc, idx)

    scaled(d_id, i_id)()
    plain()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "identity tables must give vsx_patch_gather's bits"
    reps = 20
    r = alternate({"plain": plain, "identity": scaled(d_id, i_id), "mixed": scaled(d_mix, i_mix),
                   "ops": lambda: ops.patch_gather_scaled(src, chans, tz, ty, tx, out=out)}, reps)
    say(f"kernels: n = {n} patches of (1, {ZT}, {PATCH}, {PATCH}) float32 out of 8 float32 frames (1, {Zf}, {HW}, {HW}); "
        f"{written / 1e9:.2f} GB written per launch; {WINDOWS} windows of {reps} launches")
    row("vsx_patch_gather (parent kernel), same boxes", r["plain"], written)
    row("vsx_patch_gather_scaled, identity tables", r["identity"], written)
    row("vsx_patch_gather_scaled, two scales (0.75 and 1.5) mixed", r["mixed"], written)
    row("ops.patch_gather_scaled, two scales (tables built + uploaded)", r["ops"], written)
    spread = max(r["plain"][2] - r["plain"][1], r["identity"][2] - r["identity"][1])
    diff = r["identity"][0] - r["plain"][0]
    say(f"  identity - parent = {diff * 1e3:+.1f} us; run-to-run spread (max - min of either kernel) = {spread * 1e3:.1f} us: "
        f"the bar (not slower by more than the spread) is {'MET' if diff <= spread else 'MISSED'}")
    say(f"  two scales / identity, bytes written per second = {r['identity'][0] / r['mixed'][0]:.2f}")
    say(f"  tables: {(idx.numel() * 4 + desc.numel() * 8) / 1e3:.0f} kB per batch against {written / 1e9:.2f} GB written")


# ------------------------------------------------------------------------------------------------ 3: a whole batch
def feed():
    import pandas as pd

    from viscy_amd.data import multi_experiment as me, write_hcs_plate

    small = REHEARSE
    stores = {"coarse": dict(px=0.1494 / 0.75, pz=0.174 / 0.75, Z=12 if small else 48, HW=40 if small else 320),
              "fine": dict(px=0.1494 / 1.5, pz=0.174 / 1.5, Z=20 if small else 96, HW=64 if small else 512)}
    channels = ["Phase3D", "raw GFP EX488 EM525-45"]
    rng = np.random.default_rng(3)
    rows, arrays = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        for exp, s in stores.items():
            a = rng.integers(0, 4096, size=(3, 2, s["Z"], s["HW"], s["HW"]), dtype=np.uint16)
            arrays[exp] = a
            write_hcs_plate(os.path.join(tmp, exp + ".zarr"), {"A/1/0": a}, channels)
            half = int(PATCH // 2 * 1.5) + 1 if exp == "fine" else PATCH // 2
            for track in range(BATCH // 2):
                y, x = (int(v) for v in rng.integers(half, s["HW"] - half, size=2))
                for t in range(3):
                    for ch in channels:
                        gtid = f"{exp}_A/1/0_{track}"
                        rows.append(dict(cell_id=f"{gtid}_{t}", experiment=exp, store_path=os.path.join(tmp, exp + ".zarr"), tracks_path="",
                                         fov="0", well="A/1", y=float(y), x=float(x), z=0, perturbation="mock", channel_name=ch, t=t,
                                         track_id=track, global_track_id=gtid, lineage_id=gtid, parent_track_id=-1,
                                         hours_post_perturbation=t * 0.5, interval_minutes=30.0, microscope="",
                                         marker="Phase3D" if ch == "Phase3D" else "GFP", organelle="", pixel_size_xy_um=s["px"],
                                         pixel_size_z_um=s["pz"], T_shape=3, C_shape=2, Z_shape=s["Z"], Y_shape=s["HW"], X_shape=s["HW"],
                                         norm_mean=2048.0, norm_std=1182.0, norm_median=2048.0, norm_iqr=2048.0))
        parquet = os.path.join(tmp, "cells.parquet")
        me.write_cell_index(pd.DataFrame(rows), parquet)
        registry, df = me.ExperimentRegistry.from_cell_index(
            parquet, z_window=4 if small else 32, z_extraction_window=ZT, z_focus_offset=0.3, reference_pixel_size_xy_um=0.1494,
            reference_pixel_size_z_um=0.174)
        index = me.MultiExperimentIndex(registry=registry, yx_patch_size=(PATCH, PATCH), tau_range_hours=(0.5, 1.0), cell_index_df=df)
        ds = me.MultiExperimentTripletDataset(index=index, tau_range_hours=(0.5, 1.0), channels_per_sample=1,
                                              device="cpu" if REHEARSE else "cuda")
        indices = next(iter(me.FlexibleBatchSampler(index.valid_anchors, batch_size=BATCH, stratify_by=None, seed=0)))
        ds._rng = np.random.default_rng(0)
        batch = ds.__getitems__(indices)
        assert tuple(batch["anchor"].shape) == (BATCH, 1, ZT, PATCH, PATCH) == tuple(batch["positive"].shape)

        # the reference's procedure over frames already in memory (no store read is charged to it)
        ds._rng = np.random.default_rng(0)
        boxes, _ = ds._slice_boxes(ds._va_arrays, indices, [[ds._va_arrays["channel_name"][i]] for i in indices])
        pos = ds._sample_positive_indices(indices)
        pboxes, _ = ds._slice_boxes(ds._tr_arrays, pos, [[ds._tr_arrays["channel_name"][i]] for i in pos])

        def one(b):
            a = arrays[b.experiment][b.key[2]]
            patch = a[list(b.channels), b.z_start : b.z_start + b.z_count, b.y_start : b.y_start + b.y_count, b.x_start : b.x_start + b.x_count]
            return F.interpolate(torch.from_numpy(patch.astype(np.float32))[None], size=b.target, mode="nearest-exact")[0]

        def reference(device):
            return torch.stack([one(b) for b in boxes + pboxes]).to(device)

        got = torch.cat([batch["anchor"], batch["positive"]])
        for i in list(range(8)) + list(range(len(got) - 8, len(got))):   # the tests pin the bits; here: the timed forms do the same work
            assert torch.equal(got[i].cpu().view(torch.int32), one((boxes + pboxes)[i]).view(torch.int32)), "the batch must carry the reference's bits"
        if REHEARSE:
            del got
            print("rehearsal: one host-path batch equals the restated reference procedure; nothing timed")
            return

        def clock(fn, reps):
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(times), min(times), max(times)

        def ours():
            ds._rng = np.random.default_rng(0)
            return ds.__getitems__(indices)

        del got, batch
        ours()
        t_ref, t_ours = [], []
        for _ in range(3):   # alternating rounds
            t_ours.append(clock(ours, 5))
            t_ref.append(clock(lambda: reference("cuda"), 1))
        o = (statistics.median(v[0] for v in t_ours), min(v[1] for v in t_ours), max(v[2] for v in t_ours))
        f = (statistics.median(v[0] for v in t_ref), min(v[1] for v in t_ref), max(v[2] for v in t_ref))
        say()
        say(f"a batch: {BATCH} anchors + {BATCH} positives of (1, {ZT}, {PATCH}, {PATCH}), two experiments (scales 0.75 and 1.5), uint16 stores, "
            f"warm frame cache ({ds.cache.uploads} frames resident, {ds.cache.bytes_used / 1e6:.0f} MB); host clock, ms")
        say(f"  MultiExperimentTripletDataset.__getitems__ (positives drawn, tables, one launch)   {o[0]:9.1f} ms  ({o[1]:.1f} .. {o[2]:.1f})")
        say(f"  reference procedure on the host (numpy cut, F.interpolate, stack, upload)          {f[0]:9.1f} ms  ({f[1]:.1f} .. {f[2]:.1f})")
        say(f"  reference / ours = {f[0] / o[0]:.1f}x")


if __name__ == "__main__":
    if not REHEARSE:
        assert torch.cuda.is_available(), "perf_multi_experiment_feed measures on the MI355X: no device, no number"
        say(f"device: {torch.cuda.get_device_name(0)}")
        kernels()
    feed()
    if not REHEARSE:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(lines) + "\n")
