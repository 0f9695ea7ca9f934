"""Writes tests/golden/triplet.pt: what the reference's ``TripletDataset`` (viscy_data/triplet.py) makes of a small synthetic
tracked plate.  Run on a machine that has the reference checkout; never imported by a test and never run on the GPU box.

    python tools/make_triplet_golden.py [path/to/reference/packages]

The reference module is loaded by path.  iohub, monai and tensorstore are absent: they are stubbed as
oracle/validate_against_reference.py stubs them for hcs.py, and a numpy-backed stand-in serves what the dataset asks of a
position (``zgroup.name``, ``["0"].slices / height / width / native``) and of tensorstore (``oindex``, ``translate_to``,
``stack``, ``read().result()``).  The fixture holds data only: the plate's arrays and track tables, and per case the reference's
``tracks`` / ``valid_anchors`` tables, the positive and negative rows it drew under ``np.random.seed``, the patch tensors and the
predict-mode ``index`` dicts.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.validate_against_reference import REF, _load, _stub  # noqa: E402

CHANNELS = ["Phase", "Nuclei", "Membrane"]   # storage order
SOURCE = ["Nuclei", "Phase"]                  # requested order: not the storage order
FOVS = ["A/1/0", "A/1/1", "B/2/0", "B/2/1"]
T, Z, H, W = 4, 3, 48, 40
Z_RANGE = (1, 3)
PATCH = (13, 10)   # odd in y: the extent is 12 rows
SEED = 1234


def make_plate(rng):
    """uint16 images holding 0 and 65535, and per FOV an ultrack table whose tracks start and end at different time points and
    wander across the border margin"""
    images, tables = {}, {}
    for name in FOVS:
        img = rng.integers(0, 65536, size=(T, len(CHANNELS), Z, H, W), dtype=np.uint16)
        img[:, :, :, 0, 0], img[:, :, :, -1, -1] = 0, 65535
        images[name] = img
        rows, next_id = [], 0
        for track in range(9):
            t0 = int(rng.integers(0, 2))
            t1 = min(T, t0 + int(rng.integers(2, 5)))  # most tracks reach the last time point: every anchor finds a negative there
            y, x = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
            parent = -1 if track < 5 else track - 5
            for t in range(t0, t1):
                rows.append({"track_id": track, "t": t, "id": next_id, "parent_track_id": parent, "parent_id": -1,
                             "z": int(rng.integers(0, Z)), "y": y, "x": x})
                next_id += 1
                y = int(np.clip(y + rng.integers(-3, 4), 0, H - 1))
                x = int(np.clip(x + rng.integers(-3, 4), 0, W - 1))
        tables[name] = pd.DataFrame(rows)
    norm = {ch: {"fov_statistics": {"mean": 100.0 + 10 * c, "std": 7.0 + c},
                 "timepoint_statistics": {str(t): {"mean": 50.0 + t + c, "std": 3.0 + t} for t in range(T)}}
            for c, ch in enumerate(CHANNELS)}
    return images, tables, norm


class _View:
    """what ``oindex[...]`` of the stand-in answers: the sliced array; ``translate_to[0]`` is itself (numpy has no origin)"""

    def __init__(self, a):
        self.a = a

    @property
    def translate_to(self):
        return self

    def __getitem__(self, _):
        return self


class _Native:
    def __init__(self, a):
        self.a = a
        self.oindex = self

    def __getitem__(self, key):
        t, c, z, y, x = key
        return _View(self.a[t][c][:, z][:, :, y][:, :, :, x])


class _Read:
    def __init__(self, a):
        self.a = a

    def read(self):
        return self

    def result(self):
        return self.a


class _Image:
    def __init__(self, a):
        self.frames, self.channels, self.slices, self.height, self.width = a.shape
        self.native = _Native(a)


class _Group:
    def __init__(self, name):
        self.name = name


class _Position:
    def __init__(self, name, a, norm):
        self.zgroup, self.zattrs, self._img = _Group("/" + name), {"normalization": norm}, _Image(a)

    def __getitem__(self, key):
        assert key == "0"
        return self._img

    def get_channel_index(self, ch):
        return CHANNELS.index(ch)


def load_reference(packages: str):
    for n in ("iohub", "iohub.core", "monai", "monai.data", "monai.transforms"):
        if n not in sys.modules:
            _stub(n)
    _stub("iohub.core.config", TensorStoreConfig=object)
    _stub("iohub.ngff", ImageArray=object, Position=object, open_ome_zarr=None)
    _stub("iohub.ngff.nodes", Plate=object, Position=object, Well=object)
    _stub("monai.data.utils", collate_meta_tensor=None)
    _stub("monai.data.thread_buffer", ThreadDataLoader=object)
    mt = sys.modules["monai.transforms"]
    for name in ("CenterSpatialCrop", "Cropd", "Compose", "MapTransform"):
        if not hasattr(mt, name):
            setattr(mt, name, type(name, (), {}))
    _stub("tensorstore", TensorStore=object, stack=lambda views: _Read(np.stack([v.a for v in views])))
    base = os.path.join(packages, "viscy-data", "src", "viscy_data")
    _stub("viscy_data")
    # _typing.py needs typing.NotRequired (Python >= 3.11) for aliases this path never evaluates: stubbed, as the oracle does,
    # with the one list the dataset reads taken from the file's own literal
    import ast

    with open(f"{base}/_typing.py") as f:
        columns = next(ast.literal_eval(node.value) for node in ast.parse(f.read()).body
                       if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "ULTRACK_INDEX_COLUMNS")
    _stub("viscy_data._typing", ChannelMap=dict, DictTransform=object, HCSStackIndex=tuple, NormMeta=dict, Sample=dict,
          ULTRACK_INDEX_COLUMNS=columns)
    _load("viscy_data._utils", f"{base}/_utils.py")
    _load("viscy_data.select", f"{base}/select.py")
    _stub("viscy_data.hcs", HCSDataModule=object)
    return _load("viscy_data.triplet", f"{base}/triplet.py")


def table(df) -> dict:
    df = df.drop(columns=[c for c in ("position",) if c in df.columns])
    return {"index": [int(i) for i in df.index], "columns": {c: [v if isinstance(v, str) else int(v) for v in df[c]] for c in df.columns}}


def main(packages: str) -> None:
    ref = load_reference(packages)
    images, tables, norm = make_plate(np.random.default_rng(SEED))
    golden = {"channels": CHANNELS, "source_channel": SOURCE, "fovs": FOVS, "image_size": (T, len(CHANNELS), Z, H, W),
              "z_range": Z_RANGE, "initial_yx_patch_size": PATCH, "images": {k: torch.from_numpy(v) for k, v in images.items()},
              "tracks_tables": {k: {c: [int(v) for v in df[c]] for c in df.columns} for k, df in tables.items()},
              "norm_meta": norm, "index_columns": list(sys.modules["viscy_data._typing"].ULTRACK_INDEX_COLUMNS), "cases": {}}

    def dataset(**kw):
        positions = [_Position(name, images[name], norm) for name in FOVS]
        return ref.TripletDataset(positions, [tables[name].copy() for name in FOVS], SOURCE, PATCH, slice(*Z_RANGE), **kw)

    for tag, kw in {"any_neg": dict(time_interval="any", return_negative=True), "any_noneg": dict(time_interval="any", return_negative=False),
                    "t1_neg": dict(time_interval=1, return_negative=True), "t1_noneg": dict(time_interval=1, return_negative=False)}.items():
        ds = dataset(fit=True, **kw)
        n = len(ds)
        indices = [int(i) for i in np.random.default_rng(5).permutation(n)[:9]] + [0, n - 1]
        anchor_rows = ds.valid_anchors.iloc[indices]
        case = {"kwargs": kw, "len": n, "tracks": table(ds.tracks), "valid_anchors": table(ds.valid_anchors), "indices": indices,
                "seed": SEED, "anchor_rows": table(anchor_rows)}
        if kw["time_interval"] != "any":
            case["positive_rows"] = table(ds._sample_positives(anchor_rows))
        if kw["return_negative"]:
            np.random.seed(SEED)
            case["negative_rows"] = table(ds._sample_negatives(anchor_rows))
        np.random.seed(SEED)
        sample = ds.__getitems__(indices)
        for key in ("anchor", "positive", "negative"):
            if key in sample:
                assert sample[key].dtype == torch.uint16 and sample[key].shape[1:] == (2, 2, 12, 10), (key, sample[key].shape)
                case[key] = sample[key].clone()
        case["anchor_norm_mean_Phase"] = [float(m["Phase"]["fov_statistics"]["mean"]) for m in sample["anchor_norm_meta"]]
        golden["cases"][tag] = case
        print(tag, "anchors", n, "tracks", len(ds.tracks))
    for tag, kw in {"predict": {}, "predict_cells": dict(predict_cells=True, include_fov_names=["A/1/1", "B/2/0", "A/1/1"],
                                                         include_track_ids=[2, 0, 4])}.items():
        ds = dataset(fit=False, **kw)
        indices = list(range(len(ds)))
        sample = ds.__getitems__(indices)
        golden["cases"][tag] = {"kwargs": kw, "len": len(ds), "tracks": table(ds.tracks), "indices": indices, "anchor": sample["anchor"].clone(),
                                "index": [{k: (v if isinstance(v, str) else int(v)) for k, v in d.items()} for d in sample["index"]]}
        print(tag, "cells", len(ds))
    out = os.path.join(ROOT, "tests", "golden", "triplet.pt")
    torch.save(golden, out)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else REF)
