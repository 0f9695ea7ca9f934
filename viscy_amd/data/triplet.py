"""``TripletDataset`` / ``TripletDataModule``: the tracked anchor / positive / negative feed of DynaCLR
(packages/viscy-data/src/viscy_data/triplet.py:53-588), with the patches cut on the device.

The reference reads every patch through tensorstore on the host, one read per cell and view, and uploads the stack.  Here the
time-point frames the patches come from are staged once into device memory (``feed.FrameCache``, bounded by
``device_cache_bytes``) and ONE ``vsx_patch_gather`` launch cuts a whole batch (anchor, positive and negative together) out of
them as float32 ``[n, C, Z, Yp, Xp]`` (``feed.PatchCutter``, which also serves the frames the budget cannot hold).  Without a HIP
device everything is cut on the host (``host_cut``), which is what the CPU tests compare against.

Host table work (filtering, anchors, positives, negative draws) is pandas, call for call in the reference's order, so that a
seeded run (``numpy.random.seed``) draws the same cells.

Beyond the reference: ``device_cache_bytes``.  Not built here: fusing ``NormalizeSampled`` into the gather.
``MultiExperimentDataModule`` sits on the same feed in ``multi_experiment.py``.
"""

from __future__ import annotations

import warnings
from pathlib import Path
from typing import Literal, Sequence

import numpy as np
import torch
from torch import Tensor
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from .. import ops
from .feed import (MAX_READ_THREADS, STORAGE_DTYPES, FrameCache, PatchCutter, check_storage_dtype, default_device,  # noqa: F401
                   identity, transform_channel_wise, tree_to)
from .hcs import Compose, HCSDataModule, read_norm_meta
from .ome_zarr import open_ome_zarr

ULTRACK_INDEX_COLUMNS = ["fov_name", "track_id", "t", "id", "parent_track_id", "parent_id", "z", "y", "x"]
def patch_extent(center: int, size: int) -> tuple[int, int]:
    """(start, length) of ``slice(c - s // 2, c + s // 2)``: ``2 * (s // 2)`` wide, one less than ``s`` for odd ``s``"""
    half = int(size) // 2
    return int(center) - half, 2 * half


def host_cut(frame: np.ndarray, y0: int, x0: int, yp: int, xp: int) -> np.ndarray:
    """one (C, Z, Yp, Xp) patch of a (C, Z, H, W) frame in its storage dtype; the bounds are checked as the device path checks them"""
    H, W = frame.shape[2:]
    if y0 < 0 or y0 + yp > H:
        raise ValueError(f"patch rows [{y0}, {y0 + yp}) leave the frame's [0, {H})")
    if x0 < 0 or x0 + xp > W:
        raise ValueError(f"patch columns [{x0}, {x0 + xp}) leave the frame's [0, {W})")
    return frame[:, :, y0 : y0 + yp, x0 : x0 + xp]


class TripletDataset(Dataset):
    """Anchor / positive / negative cells of tracked FOVs (triplet.py:53-287).  ``positions``: this package's OME-Zarr positions,
    ``tracks_tables``: one ultrack table per position.  Batches are formed by ``__getitems__(indices)``: float32
    ``[B, C, Z, Yp, Xp]`` tensors on ``device`` plus the per-sample ``*_norm_meta`` lists (fit), or ``anchor`` and ``index`` (predict).
    ``device``: where the batch is made (default: the current HIP device, else the CPU); ``device_cache_bytes``: the frame
    budget (``None``: every selected frame, at most half of the free device memory)."""

    def __init__(self, positions: list, tracks_tables: list, channel_names: list[str], initial_yx_patch_size: tuple[int, int],
                 z_range: slice, fit: bool = True, predict_cells: bool = False, include_fov_names: list[str] | None = None,
                 include_track_ids: list[int] | None = None, time_interval: Literal["any"] | int = "any",
                 return_negative: bool = True, device=None, device_cache_bytes: int | None = None) -> None:
        import pandas as pd

        self._pd = pd
        self.positions = list(positions)
        self.channel_names = list(channel_names)
        self.channel_indices = [positions[0].get_channel_index(ch) for ch in channel_names] if positions else []
        self.z_range, self.fit = z_range, fit
        self.yx_patch_size = tuple(initial_yx_patch_size)
        self.predict_cells = predict_cells
        self.include_fov_names = include_fov_names or []
        self.include_track_ids = include_track_ids or []
        self.time_interval = time_interval
        self.device = default_device(device)
        self._images, self._norm_meta, self._norm_resolved = {}, {}, {}
        self.tracks = self._filter_tracks(tracks_tables)
        self.tracks = self._specific_cells(self.tracks) if self.predict_cells else self.tracks
        self.valid_anchors = self._filter_anchors(self.tracks)
        self.return_negative = return_negative
        self.cache = None
        if self.device.type == "cuda":
            self.cache = FrameCache(self._load_frame, self._frame_nbytes, self.device, self._budget(device_cache_bytes))
        self._cutter = PatchCutter(self.device, self.cache, self._load_frame)

    # ------------------------------------------------------------------ tables (triplet.py:138-222)
    def _filter_tracks(self, tracks_tables):
        pd = self._pd
        filtered = []
        y_exclude, x_exclude = self.yx_patch_size[0] // 2, self.yx_patch_size[1] // 2
        if len(self.positions) != len(tracks_tables):
            raise ValueError(f"{len(self.positions)} positions for {len(tracks_tables)} tracks tables")
        for pos, tracks in zip(self.positions, tracks_tables):
            name = pos.name.strip("/")
            tracks["fov_name"] = name
            tracks["global_track_id"] = tracks["fov_name"].str.cat(tracks["track_id"].astype(str), sep="_")
            image = pos["0"]
            check_storage_dtype(image.dtype, name)
            if self.z_range.stop > image.slices:
                raise ValueError(f"Z range {self.z_range} exceeds image with Z={image.slices}")
            self._images[name], self._norm_meta[name] = image, tree_to(read_norm_meta(pos), self.device)  # once, not per batch
            y_range = (y_exclude, image.height - y_exclude)
            x_range = (x_exclude, image.width - x_exclude)
            filtered.append(tracks[tracks["y"].between(*y_range, inclusive="neither") & tracks["x"].between(*x_range, inclusive="neither")])
        return pd.concat(filtered).reset_index(drop=True)

    def _filter_anchors(self, tracks):
        if self.time_interval == "any" or not self.fit:
            return tracks
        return self._pd.concat([track[(track["t"] + self.time_interval).isin(track["t"])]
                                for (_, track) in tracks.groupby("global_track_id")])

    def _specific_cells(self, tracks):
        pd = self._pd
        specific = pd.DataFrame()
        for fov_name, track_id in zip(self.include_fov_names, self.include_track_ids):
            specific = pd.concat([specific, tracks[(tracks["fov_name"] == fov_name) & (tracks["track_id"] == track_id)]])
        return specific.reset_index(drop=True)

    def __len__(self) -> int:
        return len(self.valid_anchors)

    def _sample_positives(self, anchor_rows):
        query = anchor_rows[["global_track_id", "t"]].copy()
        query["t"] += self.time_interval
        return query.merge(self.tracks, on=["global_track_id", "t"], how="inner")

    def _sample_negative(self, anchor_row):
        if self.time_interval == "any":
            tracks = self.tracks
        else:
            tracks = self.tracks[self.tracks["t"] == anchor_row["t"] + self.time_interval]
        candidates = tracks[(tracks["global_track_id"] != anchor_row["global_track_id"])]
        # one draw from numpy's global state per anchor, in anchor order: a seeded run picks the reference's cells
        return candidates.sample(n=1).iloc[0]

    def _sample_negatives(self, anchor_rows):
        return self._pd.DataFrame([self._sample_negative(row) for _, row in anchor_rows.iterrows()]).reset_index(drop=True)

    # ------------------------------------------------------------------ frames
    def _frame_shape(self, fov: str) -> tuple[int, int, int, int]:
        img = self._images[fov]
        z0, z1, _ = self.z_range.indices(img.slices)
        return len(self.channel_indices), max(z1 - z0, 0), img.height, img.width

    def _frame_nbytes(self, key) -> int:
        return int(np.prod(self._frame_shape(key[0]))) * np.dtype(self._images[key[0]].dtype).itemsize

    def _load_frame(self, key) -> np.ndarray:
        """the (C_sel, Z_sel, H, W) block of time point ``t`` of ``fov``: only the selected channels and the Z range are read"""
        fov, t = key
        return self._images[fov].oindex[int(t), [int(i) for i in self.channel_indices], self.z_range][0]

    def total_frame_bytes(self) -> int:
        return sum(self._frame_nbytes((fov, 0)) * img.frames for fov, img in self._images.items())

    def _budget(self, device_cache_bytes: int | None) -> int:
        if device_cache_bytes is not None:
            return int(device_cache_bytes)
        free, _ = torch.cuda.mem_get_info(self.device)
        return min(self.total_frame_bytes(), free // 2)

    def _patch_specs(self, track_rows) -> tuple[list, list]:
        """per row ((fov, t), y0, x0) and the FOV's normalisation metadata"""
        specs, norms = [], []
        for fov, t, y, x in zip(track_rows["fov_name"], track_rows["t"], track_rows["y"], track_rows["x"]):
            y0, _ = patch_extent(y, self.yx_patch_size[0])
            x0, _ = patch_extent(x, self.yx_patch_size[1])
            specs.append(((fov, int(t)), y0, x0))
            norms.append(self._norm_at(fov, int(t)))
        return specs, norms

    def _norm_at(self, fov: str, t: int):
        """the FOV's metadata with ``timepoint_statistics`` resolved to time point ``t``, as ``SlidingWindowDataset`` resolves
        them: the per-sample trees then collate to (B,) tensors (the reference hands the unresolved tree on and cannot)"""
        meta = self._norm_meta[fov]
        if meta is None or not any("timepoint_statistics" in levels for levels in meta.values()):
            return meta
        got = self._norm_resolved.get((fov, t))
        if got is None:
            got = self._norm_resolved[(fov, t)] = {
                ch: {lv: (st.get(str(t), next(iter(st.values()))) if lv == "timepoint_statistics" else st) for lv, st in levels.items()}
                for ch, levels in meta.items()}
        return got

    def _cut(self, specs: list) -> Tensor:
        """float32 (n, C, Z, Yp, Xp) on ``self.device`` for ``specs``: one launch over resident frames and packed host cuts"""
        size = 2 * (self.yx_patch_size[0] // 2), 2 * (self.yx_patch_size[1] // 2)
        return self._cutter.cut(specs, [s[0] for s in specs], [(s[1], s[2]) for s in specs],
                                host_patch=lambda frame, s: host_cut(frame, s[1], s[2], *size), plain=lambda: (0, 0),
                                launch=lambda sources, origins: ops.patch_gather(sources, origins, size))

    # ------------------------------------------------------------------ batches (triplet.py:255-287)
    def __getitems__(self, indices: list[int]) -> dict:
        anchor_rows = self.valid_anchors.iloc[indices]
        specs, anchor_norms = self._patch_specs(anchor_rows)
        B = len(specs)
        sample = {"anchor_norm_meta": anchor_norms}
        keys = ["anchor"]
        if self.fit:
            if self.time_interval == "any":
                # the positive is the anchor patch itself: the same descriptors once more, no clone pass
                positive_specs, positive_norms = list(specs), anchor_norms
            else:
                positive_specs, positive_norms = self._patch_specs(self._sample_positives(anchor_rows))
            specs = specs + positive_specs
            keys.append("positive")
            sample["positive_norm_meta"] = positive_norms
            if self.return_negative:
                negative_specs, negative_norms = self._patch_specs(self._sample_negatives(anchor_rows))
                specs = specs + negative_specs
                keys.append("negative")
                sample["negative_norm_meta"] = negative_norms
        else:
            index = []
            for _, anchor_row in anchor_rows.iterrows():
                entry = {}
                for col in ULTRACK_INDEX_COLUMNS:
                    if col in anchor_row.index:
                        entry[col] = anchor_row[col]
                    elif col not in ["y", "x", "z"]:
                        raise KeyError(f"Required column '{col}' not found in data")
                index.append(entry)
            sample["index"] = index
        patches = self._cut(specs)
        if len(specs) != B * len(keys):  # an inner merge that lost or doubled a row would shift every later view
            raise RuntimeError(f"{len(specs)} patches for {len(keys)} views of {B} anchors")
        for i, key in enumerate(keys):
            sample[key] = patches[i * B : (i + 1) * B]
        return sample

    def __getitem__(self, index: int) -> dict:
        return self.__getitems__([index])


class TripletDataModule(HCSDataModule):
    """``viscy_data.triplet.TripletDataModule`` (triplet.py:290-588): keywords, defaults, exceptions and batch keys are the
    reference's.  ``num_workers``, ``persistent_workers``, ``prefetch_factor``, ``pin_memory`` and ``cache_pool_bytes`` are accepted
    and do not start processes: batches are cut on the device by the calling thread, host reads of non-resident frames use up
    to 16 threads.  ``device_cache_bytes`` (beyond the reference): bytes of device memory for resident frames, per dataset;
    ``None`` = all selected frames, at most half of the free device memory at ``setup``."""

    def __init__(self, data_path: str, tracks_path: str, source_channel: str | Sequence[str], z_range: tuple[int, int],
                 initial_yx_patch_size: tuple[int, int] = (512, 512), final_yx_patch_size: tuple[int, int] = (224, 224),
                 split_ratio: float = 0.8, batch_size: int = 16, num_workers: int = 1, normalizations: list | None = None,
                 augmentations: list | None = None, augment_validation: bool = True, fit_include_wells: list[str] | None = None,
                 fit_exclude_fovs: list[str] | None = None, predict_cells: bool = False, include_fov_names: list[str] | None = None,
                 include_track_ids: list[int] | None = None, time_interval: Literal["any"] | int = "any",
                 return_negative: bool = True, persistent_workers: bool = False, prefetch_factor: int | None = None,
                 pin_memory: bool = False, z_window_size: int | None = None, cache_pool_bytes: int = 0,
                 device_cache_bytes: int | None = None):
        if num_workers > 1:
            warnings.warn("Using more than 1 thread worker will likely degrade performance.")
        super().__init__(data_path=data_path, source_channel=source_channel, target_channel=[],
                         z_window_size=z_window_size or z_range[1] - z_range[0], split_ratio=split_ratio, batch_size=batch_size,
                         num_workers=num_workers, target_2d=False, yx_patch_size=final_yx_patch_size, normalizations=normalizations,
                         augmentations=augmentations, persistent_workers=persistent_workers, prefetch_factor=prefetch_factor,
                         pin_memory=pin_memory, normalize_on_device=False)
        self.include_fov_names = include_fov_names  # HCSDataModule keeps a set under this name; here: the predict_cells pairs
        self.z_range = slice(*z_range)
        self.tracks_path = Path(tracks_path)
        self.initial_yx_patch_size = tuple(initial_yx_patch_size)
        self._include_wells, self._exclude_fovs = fit_include_wells, fit_exclude_fovs
        self.predict_cells, self.include_track_ids = predict_cells, include_track_ids
        self.time_interval, self.return_negative = time_interval, return_negative
        self.augment_validation = augment_validation
        self._cache_pool_bytes, self.device_cache_bytes = cache_pool_bytes, device_cache_bytes
        self._augmentation_transform = Compose(self.normalizations + self.augmentations)
        self._no_augmentation_transform = Compose(self.normalizations)
        self.trainer = None
        self.device = None  # None: the current HIP device, else the CPU (TripletDataset)

    def prepare_data(self):
        pass

    def _align_tracks_tables_with_positions(self):
        """triplet.py:415-442: the FOVs of the included wells minus the excluded FOVs, each with its first ``*.csv`` cast to int"""
        import pandas as pd

        positions, tracks_tables = [], []
        plate = open_ome_zarr(self.data_path, mode="r")
        for name, fov in plate.positions():
            well = "/".join(name.split("/")[:2])
            if self._include_wells is not None and well not in self._include_wells:
                continue
            if self._exclude_fovs is not None and name.strip("/") in self._exclude_fovs:
                continue
            positions.append(fov)
            tracks_tables.append(pd.read_csv(next((self.tracks_path / name.strip("/")).glob("*.csv"))).astype(int))
        return positions, tracks_tables

    @property
    def _base_dataset_settings(self) -> dict:
        return {"channel_names": self.source_channel, "z_range": self.z_range, "time_interval": self.time_interval,
                "device": self.device, "device_cache_bytes": self.device_cache_bytes}

    def setup(self, stage: str):
        settings = self._base_dataset_settings
        if stage in ("fit", "validate"):
            positions, tracks_tables = self._align_tracks_tables_with_positions()
            order = torch.randperm(len(positions)).tolist()  # the global torch state (hcs.py:490-494)
            positions, tracks_tables = [positions[i] for i in order], [tracks_tables[i] for i in order]
            n_train = int(len(positions) * self.split_ratio)
            kw = dict(initial_yx_patch_size=self.initial_yx_patch_size, fit=True, return_negative=self.return_negative, **settings)
            self.train_dataset = TripletDataset(positions[:n_train], tracks_tables[:n_train], **kw)
            self.val_dataset = TripletDataset(positions[n_train:], tracks_tables[n_train:], **kw)
        elif stage == "test":
            raise NotImplementedError("Self-supervised model does not support testing")
        elif stage == "predict":
            positions, tracks_tables = self._align_tracks_tables_with_positions()
            self.predict_dataset = TripletDataset(positions, tracks_tables, initial_yx_patch_size=self.initial_yx_patch_size, fit=False,
                                                  predict_cells=self.predict_cells, include_fov_names=self.include_fov_names,
                                                  include_track_ids=self.include_track_ids, **settings)
        else:
            raise NotImplementedError(f"{stage} stage")

    def _loader(self, ds, batch_size, shuffle, drop_last=False):
        """batches come from ``ds.__getitems__`` in this thread (no worker process touches the device library); under
        torch.distributed the sampler is the one ``HCSDataModule._loader`` uses"""
        sampler = None
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            sampler = DistributedSampler(ds, shuffle=shuffle, seed=self.seed, drop_last=drop_last)
            shuffle = False
        return DataLoader(ds, batch_size=batch_size, num_workers=0, shuffle=shuffle, sampler=sampler, drop_last=drop_last,
                          collate_fn=identity)

    def train_dataloader(self):
        return self._loader(self.train_dataset, self.batch_size, shuffle=True, drop_last=True)

    def val_dataloader(self):
        return self._loader(self.val_dataset, self.batch_size, shuffle=False)

    def predict_dataloader(self):
        return self._loader(self.predict_dataset, self.batch_size, shuffle=False)

    def _find_transform(self, key: str):
        """triplet.py:549-559.  ``predicting`` is the trainer's flag; ``validating`` is what the fit loop tells every data module
        through ``training = False``"""
        if self.trainer is not None:
            if getattr(self.trainer, "predicting", False):
                return self._no_augmentation_transform
            if not self.training and not self.augment_validation:
                return self._no_augmentation_transform
        if key == "anchor" and self.time_interval in ("any", 0):
            return self._no_augmentation_transform
        return self._augmentation_transform

    @torch.no_grad()
    def on_after_batch_transfer(self, batch, dataloader_idx: int):
        """triplet.py:561-588"""
        if isinstance(batch, Tensor):
            return batch
        expected_spatial = (self.z_window_size, *self.yx_patch_size)
        for key in ["anchor", "positive", "negative"]:
            if key in batch:
                norm_meta_key = f"{key}_norm_meta"
                norm_meta = batch.get(norm_meta_key)
                if isinstance(norm_meta, list) and all(m is None for m in norm_meta):
                    norm_meta = None
                batch[key] = transform_channel_wise(self._find_transform(key), self.source_channel, batch[key], norm_meta)
                if norm_meta_key in batch:
                    del batch[norm_meta_key]
                actual_spatial = tuple(batch[key].shape[2:])
                if actual_spatial != expected_spatial:
                    raise ValueError(f"Spatial shape mismatch for '{key}': got {actual_spatial}, expected {expected_spatial}")
        return batch
