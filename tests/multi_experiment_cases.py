"""The synthetic two-experiment data set behind tests/golden/multi_experiment.pt: what the stores hold (arrays by a closed form,
so neither the golden file nor the tests carry them), how they are written as OME-Zarr plates, and the keyword sets the golden
generator (tools/gen_golden_multi_experiment.py) ran the reference with.  The cell-index table itself is in the golden file.

Two experiments with different pixel sizes, Z depths, storage dtypes and frame intervals:
  expA  uint16  T=5 Z=9  48 x 52   0.20 um xy, 0.40 um z, 30 min   focus metadata on the plate, no normalization attribute
  expB  float32 T=6 Z=16 64 x 60   0.10 um xy, 0.20 um z, 15 min   a normalization attribute on every position; two channels only
The table carries norm_* statistics for every row; the zattrs are what a table without those columns falls back to.
With the reference pixel sizes below the scale factors are 0.75 (expA: boxes are cut smaller and upsampled) and 1.5 (expB)."""

import json
from pathlib import Path

import numpy as np

CHANNELS = ["Phase3D", "raw GFP EX488 EM525-45", "raw mCherry EX561 EM600-37"]
MARKERS = {"Phase3D": "Phase3D", "raw GFP EX488 EM525-45": "TOMM20", "raw mCherry EX561 EM600-37": "SEC61B"}
STORES = {
    "expA": dict(store="expA.zarr", dtype="uint16", T=5, Z=9, H=48, W=52, pixel_size_xy_um=0.2, pixel_size_z_um=0.4,
                 interval_minutes=30.0, fovs={"A/1/0": "mock", "A/1/1": "mock", "B/1/0": "infected"}, z_focus_mean=5.4,
                 zattrs_norm=False, channels=CHANNELS),
    "expB": dict(store="expB.zarr", dtype="float32", T=6, Z=16, H=64, W=60, pixel_size_xy_um=0.1, pixel_size_z_um=0.2,
                 interval_minutes=15.0, fovs={"A/2/0": "mock", "B/2/0": "infected"}, z_focus_mean=None, zattrs_norm=True,
                 channels=CHANNELS[:2]),
}
REGISTRY_KW = dict(z_window=4, z_extraction_window=6, z_focus_offset=0.3, focus_channel="Phase3D",
                   reference_pixel_size_xy_um=0.15, reference_pixel_size_z_um=0.3)
YX_PATCH_SIZE = (16, 20)
TAU_RANGE_HOURS = (0.5, 1.0)

# keyword sets the generator records the reference under
SAMPLER_KW = {
    "plain": dict(batch_size=8, stratify_by=None),
    "stratified": dict(batch_size=8, stratify_by="perturbation"),
    "two_column_strata": dict(batch_size=6, stratify_by=["perturbation", "marker"]),
    "grouped": dict(batch_size=8, batch_group_by="experiment", stratify_by="perturbation"),
    "grouped_leaky_weighted": dict(batch_size=8, batch_group_by="experiment", stratify_by=None, leaky=0.25,
                                   group_weights={"expA": 1.0, "expB": 3.0}),
    "grouped_two_columns": dict(batch_size=5, batch_group_by=["experiment", "marker"], stratify_by="perturbation"),
    "temporal": dict(batch_size=8, stratify_by=None, temporal_enrichment=True, temporal_window_hours=0.5,
                     temporal_global_fraction=0.25),
    "temporal_grouped": dict(batch_size=8, batch_group_by="experiment", stratify_by="perturbation", temporal_enrichment=True,
                             temporal_window_hours=0.3, temporal_global_fraction=0.5, leaky=0.2),
    "ddp": dict(batch_size=4, stratify_by="perturbation", num_replicas=3),
}
SAMPLER_SEEDS = (0, 7)
SAMPLER_EPOCHS = 2
INDEX_KW = {
    "temporal_default_shift": dict(max_border_shift=-1),
    "temporal_no_shift": dict(max_border_shift=0),
    "temporal_shift_3": dict(max_border_shift=3),
    "self": dict(positive_cell_source="self"),
    "match_columns": dict(positive_match_columns=["perturbation", "marker"]),
    "wells_and_fovs": dict(include_wells=["A/1", "B/1", "A/2"], exclude_fovs=["A/1/1"]),
    "predict": dict(fit=False),
}
DATASET_KW = {
    "one_channel": dict(channels_per_sample=1),
    "all_channels": dict(channels_per_sample=None),
    "two_named": dict(channels_per_sample=["raw GFP EX488 EM525-45", "Phase3D"]),
    "labels": dict(channels_per_sample=1, label_columns={"condition": "perturbation", "protein": "marker"}),
}


def frame_values(spec: dict, fov: str) -> np.ndarray:
    """(T, C, Z, H, W) of the store's dtype: a closed form of the indices, different for every FOV, no two neighbours equal"""
    T, Z, H, W = spec["T"], spec["Z"], spec["H"], spec["W"]
    t, c, z, y, x = np.meshgrid(np.arange(T), np.arange(len(spec["channels"])), np.arange(Z), np.arange(H), np.arange(W), indexing="ij")
    salt = sum(ord(ch) * (i + 1) for i, ch in enumerate(fov)) + len(spec["store"])
    v = (t * 7919 + c * 10473 + z * 1299 + y * 1549 + x * 3253 + salt * 101) % 65521
    if spec["dtype"] == "uint16":
        return v.astype(np.uint16)
    return (v.astype(np.float32) - 30000.0) / 7.0


def zattrs_norm(spec: dict, fov: str) -> dict | None:
    """the ``normalization`` attribute of a position: FOV and per-time-point statistics for every channel"""
    if not spec["zattrs_norm"]:
        return None
    salt = float(sum(ord(ch) for ch in fov))
    out = {}
    for ci, ch in enumerate(spec["channels"]):
        stat = lambda k: {"mean": salt + ci + k, "std": 1.5 + ci + 0.25 * k, "median": salt - ci + k, "iqr": 2.0 + ci + 0.5 * k}  # noqa: E731
        out[ch] = {"fov_statistics": stat(0.0), "timepoint_statistics": {str(t): stat(float(t + 1)) for t in range(spec["T"])}}
    return out


def write_stores(root) -> dict:
    """the two plates under ``root``; -> {experiment: store path}"""
    from viscy_amd.data import write_hcs_plate

    paths = {}
    for name, spec in STORES.items():
        path = Path(root) / spec["store"]
        norm = {fov: zattrs_norm(spec, fov) for fov in spec["fovs"]} if spec["zattrs_norm"] else None
        write_hcs_plate(path, {fov: frame_values(spec, fov) for fov in spec["fovs"]}, spec["channels"], norm_meta=norm)
        if spec["z_focus_mean"] is not None:
            attrs = json.loads((path / ".zattrs").read_text())
            attrs["focus_slice"] = {"Phase3D": {"dataset_statistics": {"z_focus_mean": spec["z_focus_mean"]}}}
            (path / ".zattrs").write_text(json.dumps(attrs))
        paths[name] = str(path)
    return paths


def table_frame(table: dict, root):
    """the golden table (column -> list, ``store_path`` holding the store's file name) as a DataFrame under ``root``"""
    import pandas as pd

    df = pd.DataFrame(table)
    df["store_path"] = [str(Path(root) / s) for s in df["store_path"]]
    return df
