"""Writes tests/golden/multi_experiment.pt: what the reference's own ``FlexibleBatchSampler``, ``sample_tau``,
``_pick_temporal_candidate``, ``ExperimentRegistry``, ``MultiExperimentIndex`` and ``MultiExperimentTripletDataset`` compute on the
synthetic two-experiment data set of tests/multi_experiment_cases.py.

The reference modules (``viscy_data/{sampler,channel_dropout,channel_utils,cell_index,collection,_utils}.py``,
``dynaclr/data/{tau_sampling,experiment,index,dataset}.py``) are loaded from a checkout of the reference.  Third-party packages
that are not installed are stubbed to what those modules touch: ``iohub`` (``open_ome_zarr`` serving in-memory plates and
positions, ``TensorStoreConfig``), ``tensorstore`` (``oindex``, ``translate_to``, ``stack(...).read().result()``, ``Batch``; the fake
array raises where tensorstore would, on a slice that leaves the array) and ``monai`` (the names ``viscy_data/_utils.py`` imports).

Usage: ``python tools/gen_golden_multi_experiment.py --reference /path/to/reference`` (default: $VISCY_REFERENCE).  Nothing of the
reference is copied: the file holds the synthetic table, keyword sets and recorded results.
"""

import argparse
import contextlib
import importlib.util
import os
import sys
import tempfile
import types
import warnings
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "multi_experiment.pt")

from tests import multi_experiment_cases as cases  # noqa: E402

PLATES: dict = {}  # store path -> FakePlate


# ------------------------------------------------------------------------------------------------ stubs
class FakeTS:
    """what dataset.py touches of a tensorstore array"""

    def __init__(self, arr, key=None):
        self.arr, self.key = arr, key

    @property
    def shape(self):
        return self.arr.shape

    @property
    def oindex(self):
        return _OIndex(self)

    @property
    def translate_to(self):
        return _Same(self)


class _Same:
    def __init__(self, a):
        self.a = a

    def __getitem__(self, _):
        return self.a


class _OIndex:
    def __init__(self, a):
        self.a = a

    def __getitem__(self, key):
        t, chans, zs, ys, xs = key
        shape = self.a.arr.shape
        for s, dim in zip((zs, ys, xs), shape[2:]):
            if s.start < 0 or s.stop > dim or s.stop <= s.start:
                raise IndexError(f"slice [{s.start}, {s.stop}) leaves the array's [0, {dim})")
        return FakeTS(self.a.arr[t][list(chans)][:, zs, ys, xs], key=(int(t), tuple(chans), zs, ys, xs))


class _Future:
    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


class _Stacked:
    def __init__(self, parts):
        self.parts = parts

    def read(self):
        return _Future(np.stack([p.arr for p in self.parts]))


class FakeImage:
    def __init__(self, arr):
        self.arr, self.shape, self.dtype = arr, arr.shape, arr.dtype
        self.height, self.width = arr.shape[-2:]
        self.native = FakeTS(arr)


class FakePosition:
    def __init__(self, name, arr, channel_names, zattrs):
        self.channel_names, self.zattrs, self._image = list(channel_names), zattrs, FakeImage(arr)
        self.zgroup = types.SimpleNamespace(name="/" + name)

    def __getitem__(self, key):
        assert key == "0"
        return self._image

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class FakePlate:
    def __init__(self, positions: dict, zattrs: dict):
        self._positions, self.zattrs = positions, zattrs

    def positions(self):
        return iter(self._positions.items())

    def __getitem__(self, name):
        return self._positions[name.strip("/")]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def fake_open_ome_zarr(path, mode="r", **kw):
    path = str(path)
    if path in PLATES:
        return PLATES[path]
    for store, plate in PLATES.items():
        if path.startswith(store + "/"):
            return plate[path[len(store) + 1:]]
    raise FileNotFoundError(path)


def install_stubs():
    def module(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    import typing

    if not hasattr(typing, "NotRequired"):  # viscy_data/_typing.py imports it from typing (Python >= 3.11)
        class NotRequired:
            def __class_getitem__(cls, item):
                return item

        typing.NotRequired = NotRequired

    class TensorStoreConfig:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    module("iohub")
    module("iohub.ngff", open_ome_zarr=fake_open_ome_zarr, Plate=FakePlate, Position=FakePosition)
    module("iohub.core")
    module("iohub.core.config", TensorStoreConfig=TensorStoreConfig)
    module("tensorstore", TensorStore=FakeTS, Future=_Future, stack=_Stacked, Batch=contextlib.nullcontext)

    class Cropd:
        def __init__(self, keys, cropper, allow_missing_keys=False, lazy=False):
            self.keys, self.cropper = keys, cropper

    class CenterSpatialCrop:
        def __init__(self, roi_size, lazy=False):
            self.roi_size = roi_size

    module("monai")
    module("monai.data")
    module("monai.data.utils", collate_meta_tensor=lambda batch: batch)
    module("monai.transforms", Cropd=Cropd, CenterSpatialCrop=CenterSpatialCrop)


def load(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref: Path) -> dict:
    vd, dy = ref / "packages/viscy-data/src/viscy_data", ref / "applications/dynaclr/src/dynaclr"
    for pkg in ("viscy_data", "dynaclr", "dynaclr.data"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    mods = {}
    for name in ("_typing", "schemas", "collection", "cell_index", "_utils", "sampler", "channel_dropout", "channel_utils"):
        mods[name] = load(f"viscy_data.{name}", vd / f"{name}.py")
    for name in ("tau_sampling", "experiment", "index", "dataset"):
        mods[name] = load(f"dynaclr.data.{name}", dy / "data" / f"{name}.py")
    return mods


# ------------------------------------------------------------------------------------------------ the synthetic table
# per experiment and FOV: (track_id, parent_track_id, first t, last t, y, x); centres drift by one pixel per frame
TRACKS = {
    "expA": {
        "A/1/0": [(1, -1, 0, 4, 24, 26), (2, -1, 0, 2, 3, 20), (3, 2, 3, 4, 20, 45)],     # top border; right border (x + t up to 49)
        "A/1/1": [(1, -1, 0, 4, 41, 30), (2, -1, 1, 3, 20, 1), (3, -1, 0, 1, 6, 26)],      # bottom; left; two pixels off the top
        "B/1/0": [(1, -1, 0, 4, 25, 27), (2, -1, 2, 4, 30, 20), (4, -1, 0, 0, -2, 20)],    # one cell outside the image
    },
    "expB": {
        "A/2/0": [(1, -1, 0, 5, 30, 30), (2, -1, 0, 3, 20, 36), (3, 2, 4, 5, 22, 34)],
        "B/2/0": [(1, -1, 0, 5, 36, 25), (2, -1, 1, 2, 33, 33)],
    },
}


def build_table() -> dict:
    rows = []
    for exp, spec in cases.STORES.items():
        for fov, tracks in TRACKS[exp].items():
            well, pos = fov.rsplit("/", 1)
            gtid = {tid: f"{exp}_{fov}_{tid}" for tid, *_ in tracks}
            for tid, parent, t0, t1, y, x in tracks:
                lineage = gtid[parent] if parent in gtid else gtid[tid]
                for t in range(t0, t1 + 1):
                    for ci, ch in enumerate(spec["channels"]):
                        k = float(t + 10 * ci + tid)
                        rows.append(dict(
                            cell_id=f"{gtid[tid]}_{t}", experiment=exp, store_path=spec["store"], tracks_path="", fov=pos, well=well,
                            y=float(y + t), x=float(x + t), z=0, perturbation=spec["fovs"][fov], channel_name=ch, t=t, track_id=tid,
                            global_track_id=gtid[tid], lineage_id=lineage, parent_track_id=parent,
                            hours_post_perturbation=t * spec["interval_minutes"] / 60.0, interval_minutes=spec["interval_minutes"],
                            gene_name=None, reporter=None, sgRNA=None, microscope="scope" + exp[-1], marker=cases.MARKERS[ch],
                            organelle={"Phase3D": "", "TOMM20": "mitochondria", "SEC61B": "er"}[cases.MARKERS[ch]],
                            pixel_size_xy_um=spec["pixel_size_xy_um"], pixel_size_z_um=spec["pixel_size_z_um"], T_shape=spec["T"],
                            C_shape=len(spec["channels"]), Z_shape=spec["Z"], Y_shape=spec["H"], X_shape=spec["W"],
                            z_focus_mean=spec["z_focus_mean"], norm_mean=100.0 + k,
                            norm_std=3.0 + 0.5 * k, norm_median=90.0 + k,
                            norm_iqr=4.0 + 0.25 * k, norm_max=None, norm_min=None))
    return {col: [r[col] for r in rows] for col in rows[0]}


# ------------------------------------------------------------------------------------------------ recording
def plain(v):
    """tensors, numpy scalars and nested containers -> python values"""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if torch.is_tensor(v):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, np.ndarray):
        return v.tolist()
    return v


def row_ids(df) -> list:
    return [f"{c}|{ch}" for c, ch in zip(df["cell_id"].astype(str), df["channel_name"].astype(str))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VISCY_REFERENCE"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or $VISCY_REFERENCE): a checkout of the reference")
    warnings.simplefilter("ignore", FutureWarning)
    install_stubs()
    ref = load_reference(Path(args.reference))
    from viscy_amd.data.multi_experiment import write_cell_index

    golden = {"table": build_table()}
    with tempfile.TemporaryDirectory() as tmp:
        for exp, spec in cases.STORES.items():
            store = str(Path(tmp) / spec["store"])
            os.makedirs(store)
            zattrs = {}
            if spec["z_focus_mean"] is not None:
                zattrs["focus_slice"] = {"Phase3D": {"dataset_statistics": {"z_focus_mean": spec["z_focus_mean"]}}}
            positions = {}
            for fov in spec["fovs"]:
                pz = {}
                norm = cases.zattrs_norm(spec, fov)
                if norm is not None:
                    pz["normalization"] = norm
                positions[fov] = FakePosition(fov, cases.frame_values(spec, fov), spec["channels"], pz)
            PLATES[store] = FakePlate(positions, zattrs)
        parquet = str(Path(tmp) / "cells.parquet")
        write_cell_index(cases.table_frame(golden["table"], tmp), parquet)

        ExperimentRegistry = ref["experiment"].ExperimentRegistry
        MultiExperimentIndex = ref["index"].MultiExperimentIndex
        Dataset = ref["dataset"].MultiExperimentTripletDataset
        registry, df = ExperimentRegistry.from_cell_index(parquet, **cases.REGISTRY_KW)
        golden["registry"] = plain({
            "z_ranges": registry.z_ranges, "scale_factors": registry.scale_factors,
            "tau_range_frames": {e.name: registry.tau_range_frames(e.name, cases.TAU_RANGE_HOURS) for e in registry.experiments},
            "source_channel_labels": registry.source_channel_labels,
            "channels": {e.name: [(c.name, c.marker) for c in e.channels] for e in registry.experiments},
            "channel_names": {e.name: e.channel_names for e in registry.experiments},
            "perturbation_wells": {e.name: e.perturbation_wells for e in registry.experiments},
            "subset": [e.name for e in registry.subset(["expB"]).experiments]})

        def make_index(kw):
            return MultiExperimentIndex(registry=registry, yx_patch_size=cases.YX_PATCH_SIZE, tau_range_hours=cases.TAU_RANGE_HOURS,
                                        cell_index_df=df, **kw)

        golden["index"] = {}
        for name, kw in cases.INDEX_KW.items():
            ix = make_index(kw)
            golden["index"][name] = {
                "tracks": row_ids(ix.tracks), "y_clamp": plain(ix.tracks["y_clamp"].to_numpy()),
                "x_clamp": plain(ix.tracks["x_clamp"].to_numpy()), "valid_anchors": row_ids(ix.valid_anchors),
                "max_border_shift": int(ix.max_border_shift), "summary": ix.summary(),
                "experiment_groups": plain(ix.experiment_groups), "condition_groups": plain(ix.condition_groups)}

        # ---- sampler
        anchors = make_index(cases.INDEX_KW["temporal_default_shift"]).valid_anchors
        Sampler = ref["sampler"].FlexibleBatchSampler
        golden["sampler"] = {}
        for name, kw in cases.SAMPLER_KW.items():
            per_seed = {}
            for seed in cases.SAMPLER_SEEDS:
                per_rank = []
                for rank in range(kw.get("num_replicas", 1)):
                    s = Sampler(anchors, seed=seed, rank=rank, **kw)
                    epochs = [list(s) for _ in range(cases.SAMPLER_EPOCHS)]
                    s.set_epoch(5)
                    per_rank.append({"length": len(s), "epochs": epochs, "after_set_epoch_5": list(s)})
                per_seed[seed] = per_rank
            golden["sampler"][name] = per_seed

        # ---- tau and temporal candidates
        golden["sample_tau"] = []
        for tau_min, tau_max, decay, seed in ((1, 2, 2.0, 0), (2, 4, 2.0, 1), (1, 6, 0.0, 2), (-3, 3, 1.5, 3), (4, 4, 2.0, 4)):
            rng = np.random.default_rng(seed)
            golden["sample_tau"].append({"args": (tau_min, tau_max, decay), "seed": seed,
                                         "draws": [ref["tau_sampling"].sample_tau(tau_min, tau_max, rng, decay) for _ in range(24)]})
        markers = np.array(["a", "b", "a", "b", "a", "b", "a", "a", "b", "b"], dtype=object)
        timepoints = {0: [0, 1], 1: [2, 3], 2: [4, 5, 6], 4: [7, 8, 9]}
        golden["pick_temporal"] = {"timepoints": timepoints, "markers": markers.tolist(), "cases": []}
        for anchor_t, tau_min, tau_max, use_markers, anchor_marker, seed in (
                (0, 1, 2, False, None, 0), (0, 1, 2, True, "a", 1), (0, 1, 2, True, "b", 2), (1, 2, 3, True, "a", 3),
                (2, 1, 1, False, None, 4), (2, -2, 2, True, "b", 5), (4, 1, 3, True, "a", 6), (0, 3, 4, True, "c", 7)):
            rng = np.random.default_rng(seed)
            picks = [ref["dataset"]._pick_temporal_candidate(timepoints, anchor_t, tau_min, tau_max, 2.0, rng,
                                                              markers if use_markers else None, anchor_marker) for _ in range(12)]
            golden["pick_temporal"]["cases"].append({"args": (anchor_t, tau_min, tau_max, use_markers, anchor_marker),
                                                     "seed": seed, "picks": picks})

        # ---- dataset: boxes, norm meta, resampled patches
        golden["dataset"] = {}
        for name, kw in cases.DATASET_KW.items():
            ix = make_index(cases.INDEX_KW["temporal_default_shift"])
            ds = Dataset(index=ix, fit=True, tau_range_hours=cases.TAU_RANGE_HOURS, **kw)
            va = ix.valid_anchors
            n = len(va)
            if ds._channel_mode == "from_index":
                forced = [[ds._va_arrays["channel_name"][i]] for i in range(n)]
            elif ds._channel_mode == "fixed":
                forced = [ds._fixed_channel_names] * n
            else:
                forced = [None] * n
            boxes, norms = [], []
            for i in range(n):
                patch, norm, scale, target = ds._slice_patch(ds._va_arrays, i, forced_channel_names=forced[i])
                t, chans, zs, ys, xs = patch.key
                boxes.append([t, list(chans), zs.start, zs.stop, ys.start, ys.stop, xs.start, xs.stop, *target])
                norms.append(plain(norm))
            exp_of = va["experiment"].astype(str).to_numpy()
            a_rows, b_rows = np.flatnonzero(exp_of == "expA"), np.flatnonzero(exp_of == "expB")
            rec = {"valid_anchors": row_ids(va), "boxes": boxes, "norm_meta": norms,
                   "label_encoders": plain({k: {"column": c, "encoder": e} for k, (c, e) in ds._label_encoders.items()})}
            groups = {"expA": a_rows[[0, -1]].tolist(), "expB": b_rows[[0, -1]].tolist()}
            if name != "all_channels":
                groups["mixed"] = [int(a_rows[len(a_rows) // 2]), int(b_rows[len(b_rows) // 2]), int(a_rows[-2])]
            rec["patches"] = {}
            for gname, rows in ({} if name == "labels" else groups).items():
                fc = None if forced[0] is None else [forced[i] for i in rows]
                tensor, _ = ds._slice_patches(ds._va_arrays, rows, fc)
                rec["patches"][gname] = {"rows": rows, "patches": tensor.clone()}
            if name == "all_channels":
                try:
                    ds._slice_patches(ds._va_arrays, [int(a_rows[0]), int(b_rows[0])], None)
                except RuntimeError as e:
                    rec["mixed_channel_error"] = str(e)
            rows = [0, n // 2, n - 1]
            rec["meta"] = {"rows": rows, "records": plain(ds._extract_meta(va.iloc[rows]))}
            golden["dataset"][name] = rec

        # ---- norm meta from the positions' zattrs: a table without norm_* columns (expA has no such attribute: None)
        bare = df.drop(columns=[c for c in df.columns if c.startswith("norm_")])
        golden["zattrs_norm_meta"] = {}
        for name in ("one_channel", "all_channels", "two_named"):
            ix = MultiExperimentIndex(registry=registry, yx_patch_size=cases.YX_PATCH_SIZE, tau_range_hours=cases.TAU_RANGE_HOURS,
                                      cell_index_df=bare)
            ds = Dataset(index=ix, fit=True, tau_range_hours=cases.TAU_RANGE_HOURS, **cases.DATASET_KW[name])
            n = len(ix.valid_anchors)
            if ds._channel_mode == "from_index":
                forced = [[ds._va_arrays["channel_name"][i]] for i in range(n)]
            else:
                forced = [ds._fixed_channel_names if ds._channel_mode == "fixed" else None] * n
            golden["zattrs_norm_meta"][name] = {"valid_anchors": row_ids(ix.valid_anchors), "norm_meta": [
                plain(ds._build_norm_meta(ds._va_arrays, i, forced[i])) for i in range(n)]}

        # ---- predict
        ix = make_index(cases.INDEX_KW["predict"])
        ds = Dataset(index=ix, fit=False, tau_range_hours=cases.TAU_RANGE_HOURS, channels_per_sample=1)
        rows = [0, len(ix.valid_anchors) // 3, len(ix.valid_anchors) - 1]
        batch = ds.__getitems__(rows)
        golden["predict"] = {"rows": rows, "index": plain(batch["index"]), "anchor": batch["anchor"].clone(),
                             "keys": sorted(batch), "anchor_meta": plain(batch["anchor_meta"])}

    torch.save(golden, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(golden['table']['cell_id'])} table rows")


if __name__ == "__main__":
    main()
