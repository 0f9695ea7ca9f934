"""``MultiExperimentDataModule``: the DynaCLR feed over a cell-index parquet that spans experiments of different pixel sizes,
Z ranges and channel sets (applications/dynaclr/src/dynaclr/data/{experiment,index,dataset,datamodule}.py,
packages/viscy-data/src/viscy_data/{sampler,channel_dropout,channel_utils}.py), with the patches cut and resampled on the device.

The reference reads one native box per cell and view through tensorstore, resamples each on the host with
``F.interpolate(mode="nearest-exact")``, stacks and uploads.  Here the time-point frames stay resident in device memory
(``feed.FrameCache``) and ONE ``vsx_patch_gather_scaled`` launch forms anchor and positive together (``feed.PatchCutter``, which
also serves the frames the budget cannot hold): every patch names its channels and its source planes, rows and columns through
index tables, and the tables ARE the resampling (``nearest_exact_index`` takes the map from CPU torch itself, per ``(in, out)``
pair, so the kernel restates no formula).  Without a HIP device everything goes through ``host_gather`` with the same tables,
which is what the CPU tests compare against the reference's recorded patches.

Host table work is pandas / numpy in the reference's order; ``FlexibleBatchSampler`` draws what the reference draws for a seed.

Beyond the reference: ``device_cache_bytes``.  Different from it: patches are float32 on the device for every storage dtype (the
reference leaves unscaled integer patches in their storage dtype until the first transform); the dataset's positive draws
come from its own unseeded ``numpy.random.Generator`` as the reference's do, so only the sampler is reproducible draw for draw;
a row whose ``norm_mean`` is null (NaN of any float type) takes its statistics from the FOV's ``normalization`` attribute, where
the reference, testing ``isinstance(norm_mean, float)``, hands a float32 NaN on as the statistics; null ``Y_shape`` / ``X_shape``
fall back to the image sizes in the stores.
Not built (each raises ``NotImplementedError`` naming itself, or is absent): building a cell index from zarr and tracking CSVs
(``_load_all_experiments``, ``build_*_cell_index``, ``preprocess_cell_index``, ``convert_ops_parquet``), ``_reconstruct_lineage``,
collection YAML authoring, ``return_negative``, fusing ``NormalizeSampled`` into the gather.
"""

from __future__ import annotations

import functools
import logging
import math
import re
from collections import defaultdict
from dataclasses import dataclass, field
from pathlib import Path
from typing import Iterator

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.utils.data import DataLoader, Dataset, Sampler

from .. import ops
from .feed import FrameCache, PatchCutter, check_storage_dtype, default_device, identity, transform_channel_wise
from .hcs import Compose, read_norm_meta
from .ome_zarr import open_ome_zarr
from .triplet import ULTRACK_INDEX_COLUMNS

try:  # pragma: no cover
    from lightning.pytorch import LightningDataModule as _DMBase
except Exception:  # noqa: BLE001
    _DMBase = object

_logger = logging.getLogger(__name__)

__all__ = ["ChannelDropout", "ExperimentRegistry", "FlexibleBatchSampler", "MultiExperimentDataModule", "MultiExperimentIndex",
           "MultiExperimentTripletDataset", "host_gather", "nearest_exact_index", "parse_channel_name", "sample_tau"]


# ------------------------------------------------------------------------------------------------ the resampling map
@functools.lru_cache(maxsize=None)
def _nearest_exact(in_size: int, out_size: int) -> np.ndarray:
    if not (0 < in_size <= 2 ** 24 and out_size > 0):
        raise ValueError(f"nearest_exact_index: sizes ({in_size}, {out_size}) must be positive, the source at most 2**24")
    src = torch.arange(in_size, dtype=torch.float32).reshape(1, 1, in_size)  # float32: what ``_rescale_patch`` interpolates
    idx = F.interpolate(src, size=out_size, mode="nearest-exact").reshape(out_size).to(torch.int64).numpy()
    idx.setflags(write=False)
    return idx


def nearest_exact_index(in_size: int, out_size: int) -> np.ndarray:
    """int64 (out_size,): the source index ``F.interpolate(x.float(), size=out_size, mode="nearest-exact")`` reads for every output
    position along an axis of ``in_size`` elements.  Taken from CPU torch itself, by interpolating an ``arange``, and cached per
    pair: no closed form in float32, float64 or exact arithmetic agrees with torch on every pair.  The array is read-only and the
    same object for the same pair."""
    return _nearest_exact(int(in_size), int(out_size))


def host_gather(frame: np.ndarray, channels, zs, ys, xs) -> np.ndarray:
    """``frame[channels][:, zs][:, :, ys][:, :, :, xs]`` of a (Cf, Zf, H, W) array in its storage dtype, the tables checked as
    ``ops.patch_gather_scaled`` checks them"""
    tables = [np.asarray(t, dtype=np.int64) for t in (channels, zs, ys, xs)]
    for axis, t, dim in zip(("channel", "z", "y", "x"), tables, frame.shape):
        if t.size == 0 or t.min() < 0 or t.max() >= dim:
            raise ValueError(f"host_gather: {axis} table spans [{t.min() if t.size else 0}, {t.max() if t.size else -1}], "
                             f"which leaves the frame's [0, {dim})")
    return frame[np.ix_(*tables)]


# ------------------------------------------------------------------------------------------------ small reference pieces
def sample_tau(tau_min: int, tau_max: int, rng: np.random.Generator, decay_rate: float = 2.0) -> int:
    """tau_sampling.py: one temporal offset in [tau_min, tau_max], p ~ exp(-decay_rate * (tau - tau_min) / (tau_max - tau_min))"""
    if tau_min == tau_max:
        return int(tau_min)
    taus = np.arange(tau_min, tau_max + 1)
    weights = np.exp(-decay_rate * (taus - tau_min) / (tau_max - tau_min))
    weights /= weights.sum()
    return int(rng.choice(taus, p=weights))


class ChannelDropout(nn.Module):
    """channel_dropout.py: zero whole channels of (B, C, Z, Y, X) per sample with probability ``p``, in training mode only"""

    def __init__(self, channels: list[int], p: float = 0.5) -> None:
        super().__init__()
        self.channels, self.p = channels, p

    def forward(self, x: Tensor) -> Tensor:
        if not self.training or self.p == 0.0:
            return x
        out = x.clone()
        for ch in self.channels:
            mask = torch.rand(out.shape[0], device=out.device) < self.p
            out[mask, ch] = 0.0
        return out


def parse_channel_name(name: str) -> dict:
    """channel_utils.py: ``channel_type`` ("fluorescence" | "virtual_stain" | "labelfree" | "unknown") and, for fluorescence
    labels, ``filter_cube`` / ``excitation_nm`` / ``emission_nm`` parsed from a zarr channel label"""
    result: dict = {}
    lower = name.lower()
    fl = re.match(r"raw\s+(\w+)\s+EX(\d+)\s+EM(\d+)(?:-(\d+))?", name, re.IGNORECASE)
    if fl:
        return {"channel_type": "fluorescence", "filter_cube": fl.group(1), "excitation_nm": int(fl.group(2)),
                "emission_nm": int(fl.group(3))}
    if any(kw in lower for kw in ("prediction", "virtual", "vs_")):  # before label-free: substring collisions
        result["channel_type"] = "virtual_stain"
        return result
    if any(kw in lower for kw in ("phase", "brightfield", "retardance")) or any(
            re.search(p, lower) for p in (r"\bbf(\b|_)", r"\bdic\b", r"\bpol\b", r"\bphc\b")):
        result["channel_type"] = "labelfree"
        return result
    ex_em = re.search(r"EX(\d+)\s*EM(\d+)", name, re.IGNORECASE)
    if ex_em:
        return {"channel_type": "fluorescence", "excitation_nm": int(ex_em.group(1)), "emission_nm": int(ex_em.group(2))}
    result["channel_type"] = "unknown"
    return result


def _pick_temporal_candidate(timepoints: dict, anchor_t: int, tau_min: int, tau_max: int, tau_decay_rate: float,
                             rng: np.random.Generator, tr_marker_arr, anchor_marker) -> int | None:
    """dataset.py:42-82: one tracks index at ``anchor_t + tau``: the sampled tau first, then every tau of the window in order"""

    def _filter_and_pick(cand_indices):
        if not cand_indices:
            return None
        if tr_marker_arr is not None:
            idx_arr = np.asarray(cand_indices, dtype=np.int64)
            filtered = idx_arr[tr_marker_arr[idx_arr] == anchor_marker]
            if len(filtered) > 0:
                return int(filtered[rng.integers(len(filtered))])
        return int(cand_indices[rng.integers(len(cand_indices))])

    result = _filter_and_pick(timepoints.get(anchor_t + sample_tau(tau_min, tau_max, rng, tau_decay_rate), []))
    if result is not None:
        return result
    for tau in range(tau_min, tau_max + 1):
        if tau == 0:
            continue
        result = _filter_and_pick(timepoints.get(anchor_t + tau, []))
        if result is not None:
            return result
    return None


# ------------------------------------------------------------------------------------------------ sampler (sampler.py)
class FlexibleBatchSampler(Sampler):
    """``viscy_data.sampler.FlexibleBatchSampler``: batches of row positions of ``valid_anchors`` built by a cascade: pick one
    group (``batch_group_by``), mix in a ``leaky`` fraction from the other groups, then draw the rest with temporal enrichment,
    or balanced over the strata of ``stratify_by``, or plainly.  One ``numpy.random.default_rng(seed + epoch)`` per epoch; every
    rank builds every batch and yields its own, so the draws are the reference's for any topology."""

    def __init__(self, valid_anchors, batch_size: int = 128, batch_group_by: str | list[str] | None = None, leaky: float = 0.0,
                 group_weights: dict[str, float] | None = None, stratify_by: str | list[str] | None = "perturbation",
                 temporal_enrichment: bool = False, temporal_window_hours: float = 2.0, temporal_global_fraction: float = 0.3,
                 num_replicas: int = 1, rank: int = 0, seed: int = 0, drop_last: bool = True) -> None:
        if isinstance(batch_group_by, str):
            batch_group_by = [batch_group_by]
        if isinstance(stratify_by, str):
            stratify_by = [stratify_by]
        for what, cols in (("batch_group_by", batch_group_by), ("stratify_by", stratify_by)):
            if cols is not None:
                missing = [c for c in cols if c not in valid_anchors.columns]
                if missing:
                    raise ValueError(f"{what}={cols} requires columns {missing} in valid_anchors, but columns are: "
                                     f"{list(valid_anchors.columns)}")
        if temporal_enrichment and "hours_post_perturbation" not in valid_anchors.columns:
            raise ValueError("temporal_enrichment=True requires 'hours_post_perturbation' column in valid_anchors, but columns "
                             f"are: {list(valid_anchors.columns)}")
        self.valid_anchors, self.batch_size = valid_anchors, batch_size
        self.batch_group_by, self.leaky, self.group_weights, self.stratify_by = batch_group_by, leaky, group_weights, stratify_by
        self.temporal_enrichment, self.temporal_window_hours = temporal_enrichment, temporal_window_hours
        self.temporal_global_fraction = temporal_global_fraction
        self.num_replicas, self.rank, self.seed, self.drop_last = num_replicas, rank, seed, drop_last
        self.epoch = 0
        if self.temporal_enrichment:
            self._hpi_values = valid_anchors["hours_post_perturbation"].to_numpy()
        self._precompute_groups()

    @staticmethod
    def _indices_by_key(keys) -> dict[str, np.ndarray]:
        import pandas as pd

        if isinstance(keys.dtype, pd.CategoricalDtype):
            codes = keys.cat.codes.to_numpy()
            out = {}
            for c, name in enumerate(list(keys.cat.categories)):
                rows = np.flatnonzero(codes == c)
                if len(rows) > 0:
                    out[str(name)] = rows
            return out
        return {str(name): group.to_numpy() for name, group in keys.groupby(keys).groups.items()}

    @staticmethod
    def _compute_strat_keys(df, columns: list[str]):
        if len(columns) == 1:
            return df[columns[0]]
        return df[columns].astype(str).agg("|".join, axis=1)

    def _precompute_groups(self) -> None:
        if self.batch_group_by is not None:
            self._group_indices = self._indices_by_key(self._compute_strat_keys(self.valid_anchors, self.batch_group_by))
            self._group_names = list(self._group_indices.keys())
        else:
            self._group_indices, self._group_names = {}, []
        self._strat_indices, self._group_strat_indices, self._strat_names = {}, {}, []
        if self.stratify_by is not None:
            self._strat_indices = self._indices_by_key(self._compute_strat_keys(self.valid_anchors, self.stratify_by))
            self._strat_names = list(self._strat_indices.keys())
            if self.batch_group_by is not None:
                for grp, g_idx in self._group_indices.items():
                    for strat_key, s_idx in self._strat_indices.items():
                        common = np.intersect1d(g_idx, s_idx, assume_unique=True)
                        if len(common) > 0:
                            self._group_strat_indices[(grp, strat_key)] = common
        self._all_indices = np.arange(len(self.valid_anchors))
        if self.batch_group_by is not None:
            total = len(self.valid_anchors)
            if self.group_weights is not None:
                raw = np.array([self.group_weights.get(n, 0.0) for n in self._group_names])
                self._group_probs = raw / raw.sum()
            else:
                self._group_probs = np.array([len(self._group_indices[n]) / total for n in self._group_names])
            for name, indices in self._group_indices.items():
                if len(indices) < self.batch_size:
                    _logger.warning("Group '%s' has %d samples, fewer than batch_size=%d. Will use replacement sampling for this "
                                    "group.", name, len(indices), self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self) -> int:
        return math.ceil((len(self.valid_anchors) // self.batch_size) / self.num_replicas)

    def __iter__(self) -> Iterator[list[int]]:
        seed_offset = self.epoch
        self.epoch += 1  # at the start: an iteration cut short still advances
        rng = np.random.default_rng(self.seed + seed_offset)
        for i in range(len(self.valid_anchors) // self.batch_size):
            batch = self._build_one_batch(rng)
            if i % self.num_replicas == self.rank:
                yield batch

    def _build_one_batch(self, rng: np.random.Generator) -> list[int]:
        chosen_group = None
        if self.batch_group_by is not None:
            chosen_group = rng.choice(self._group_names, p=self._group_probs)
            pool = self._group_indices[chosen_group]
        else:
            pool = self._all_indices
        leak_samples = None
        if self.batch_group_by is not None and self.leaky > 0.0 and chosen_group is not None:
            n_leak = int(self.batch_size * self.leaky)
            n_primary = self.batch_size - n_leak
            if n_leak > 0:
                other = np.concatenate([v for k, v in self._group_indices.items() if k != chosen_group])
                if len(other) > 0:
                    leak_samples = rng.choice(other, size=min(n_leak, len(other)), replace=len(other) < n_leak)
        else:
            n_primary = self.batch_size
        if self.temporal_enrichment:
            primary = self._enrich_temporal(pool, n_primary, rng, chosen_group)
        elif self.stratify_by is not None:
            primary = self._sample_stratified(pool, n_primary, chosen_group, rng)
        else:
            primary = rng.choice(pool, size=n_primary, replace=len(pool) < n_primary)
        combined = np.concatenate([primary, leak_samples]) if leak_samples is not None and len(leak_samples) > 0 else primary
        return [int(x) for x in combined]

    def _enrich_temporal(self, pool: np.ndarray, n_target: int, rng: np.random.Generator, chosen_group) -> np.ndarray:
        hpi = self._hpi_values
        focal_hpi = rng.choice(np.unique(hpi[pool]))
        focal_mask = np.abs(hpi[pool] - focal_hpi) <= self.temporal_window_hours
        focal_pool, global_pool = pool[focal_mask], pool[~focal_mask]
        n_global = int(n_target * self.temporal_global_fraction)
        n_focal = n_target - n_global

        def draw(n, first):
            if n > 0 and len(first) > 0:
                return rng.choice(first, size=n, replace=len(first) < n)
            if n > 0:
                return rng.choice(pool, size=n, replace=len(pool) < n)
            return np.array([], dtype=int)

        focal_samples = draw(n_focal, focal_pool)
        global_samples = draw(n_global, global_pool)
        return np.concatenate([focal_samples, global_samples])

    def _sample_stratified(self, pool: np.ndarray, n_samples: int, chosen_group, rng: np.random.Generator) -> np.ndarray:
        if chosen_group is not None:
            strata = [key for (grp, key) in self._group_strat_indices if grp == chosen_group]
            pools = {key: self._group_strat_indices.get((chosen_group, key), np.array([], dtype=int)) for key in strata}
        else:
            strata = self._strat_names
            pools = {key: self._strat_indices.get(key, np.array([], dtype=int)) for key in strata}
        if not strata:
            return rng.choice(pool, size=n_samples, replace=len(pool) < n_samples)
        ratios = self._compute_ratios(strata)
        parts, remaining = [], n_samples
        for i, key in enumerate(strata):
            strat_pool = pools[key]
            if len(strat_pool) == 0:
                continue
            if i == len(strata) - 1:
                n_stratum = remaining
            else:
                n_stratum = int(n_samples * ratios[key])
                remaining -= n_stratum
            parts.append(rng.choice(strat_pool, size=n_stratum, replace=len(strat_pool) < n_stratum))
        if parts:
            return np.concatenate(parts)
        return rng.choice(pool, size=n_samples, replace=len(pool) < n_samples)

    @staticmethod
    def _compute_ratios(strata: list[str]) -> dict[str, float]:
        return {s: 1.0 / len(strata) for s in strata}


# ------------------------------------------------------------------------------------------------ registry (experiment.py)
# the parquet contract (viscy_data/cell_index.py CELL_INDEX_SCHEMA): column -> arrow type name
CELL_INDEX_COLUMNS = (
    ("cell_id", "string"), ("experiment", "string"), ("store_path", "string"), ("tracks_path", "string"), ("fov", "string"),
    ("well", "string"), ("y", "float32"), ("x", "float32"), ("z", "int16"), ("perturbation", "string"), ("channel_name", "string"),
    ("t", "int32"), ("track_id", "int32"), ("global_track_id", "string"), ("lineage_id", "string"), ("parent_track_id", "int32"),
    ("hours_post_perturbation", "float32"), ("interval_minutes", "float32"), ("gene_name", "string"), ("reporter", "string"),
    ("sgRNA", "string"), ("microscope", "string"), ("marker", "string"), ("organelle", "string"), ("pixel_size_xy_um", "float32"),
    ("pixel_size_z_um", "float32"), ("T_shape", "int32"), ("C_shape", "int32"), ("Z_shape", "int32"), ("Y_shape", "int32"),
    ("X_shape", "int32"), ("z_focus_mean", "float32"), ("norm_mean", "float32"), ("norm_std", "float32"), ("norm_median", "float32"),
    ("norm_iqr", "float32"), ("norm_max", "float32"), ("norm_min", "float32"))
_CATEGORICAL_COLUMNS = ("experiment", "marker", "store_path", "microscope", "organelle", "reporter", "channel_name")


def cell_index_schema():
    import pyarrow as pa

    return pa.schema([(name, getattr(pa, kind)()) for name, kind in CELL_INDEX_COLUMNS])


def read_cell_index(path):
    """cell_index.py:184-229: the parquet under the canonical schema as a DataFrame, low-cardinality strings as Categorical"""
    import pyarrow.parquet as pq

    df = pq.read_table(str(path), schema=cell_index_schema()).to_pandas(use_threads=True)
    for col in _CATEGORICAL_COLUMNS:
        if col in df.columns:
            df[col] = df[col].astype("category")
    return df


def write_cell_index(df, path) -> None:
    """cell_index.py:150-181 without the validation: missing schema columns are written as nulls"""
    import pyarrow as pa
    import pyarrow.parquet as pq

    df = df.copy()
    for name, _ in CELL_INDEX_COLUMNS:
        if name not in df.columns:
            df[name] = None
    pq.write_table(pa.Table.from_pandas(df, schema=cell_index_schema(), preserve_index=False), str(path))


@dataclass
class ChannelEntry:
    name: str
    marker: str
    wells: list = field(default_factory=list)


@dataclass
class ExperimentEntry:
    """collection.py ``ExperimentEntry``: one experiment of a collection"""

    name: str
    data_path: str
    tracks_path: str
    channels: list = field(default_factory=list)
    channel_names: list = field(default_factory=list)
    perturbation_wells: dict = field(default_factory=dict)
    interval_minutes: float = 30.0
    start_hpi: float = 0.0
    marker: str = ""
    organelle: str = ""
    microscope: str = ""
    pixel_size_xy_um: float | None = None
    pixel_size_z_um: float | None = None
    date: str = ""
    moi: float = 0.0
    exclude_fovs: list = field(default_factory=list)


@dataclass
class Collection:
    name: str
    experiments: list
    description: str = ""
    datasets_root: str | None = None
    provenance: object = None
    fov_records: list = field(default_factory=list)


@dataclass
class ExperimentRegistry:
    """``dynaclr.data.experiment.ExperimentRegistry``: the validated experiments of a collection with per-experiment ``z_ranges``
    (from the plate's ``focus_slice`` metadata, ``z_extraction_window`` and ``z_focus_offset``) and ``scale_factors``
    (reference pixel size / experiment pixel size, per axis).  Built from a cell-index parquet (``from_cell_index``)."""

    collection: Collection
    z_window: int | None = None
    z_extraction_window: int | None = None
    z_focus_offset: float = 0.5
    focus_channel: str | None = None
    reference_pixel_size_xy_um: float | None = None
    reference_pixel_size_z_um: float | None = None
    z_ranges: dict = field(init=False)
    scale_factors: dict = field(init=False)
    _name_map: dict = field(init=False, repr=False, compare=False)

    def __post_init__(self) -> None:
        experiments = self.collection.experiments
        if not experiments:
            raise ValueError("Empty experiments list: at least one experiment is required.")
        seen: set = set()
        for e in experiments:
            if e.name in seen:
                raise ValueError(f"Duplicate experiment name '{e.name}'. Each experiment must have a unique name.")
            seen.add(e.name)
        self._name_map = {e.name: e for e in experiments}
        z_extract = self.z_extraction_window or self.z_window
        z_ranges = {}
        for exp in experiments:
            if exp.interval_minutes < 0:
                raise ValueError(f"Experiment '{exp.name}': interval_minutes must be non-negative, got {exp.interval_minutes}.")
            if not exp.perturbation_wells:
                raise ValueError(f"Experiment '{exp.name}': perturbation_wells must not be empty.")
            if not Path(exp.data_path).exists():
                raise ValueError(f"Experiment '{exp.name}': data_path does not exist: {exp.data_path}")
            with open_ome_zarr(exp.data_path, mode="r") as plate:
                first_position = next(iter(plate.positions()))[1]
                zarr_channels = list(first_position.channel_names)
                z_total = first_position["0"].shape[2]
                focus_data = plate.zattrs.get("focus_slice", {})
            exp.channel_names = zarr_channels
            missing_channels = [ch.name for ch in exp.channels if ch.name not in zarr_channels]
            if missing_channels:
                raise ValueError(f"Experiment '{exp.name}': channels {missing_channels} not found in zarr. "
                                 f"Available: {zarr_channels}.")
            if z_extract is None:
                z_ranges[exp.name] = (0, z_total)
            else:
                focus_ch = self.focus_channel or (exp.channels[0].name if exp.channels else None)
                ch_focus = focus_data.get(focus_ch, {}) if focus_ch else {}
                z_focus_mean = ch_focus.get("dataset_statistics", {}).get("z_focus_mean")
                z_center = int(round(z_focus_mean)) if z_focus_mean is not None else z_total // 2
                effective_extract = min(z_extract, z_total)
                z_below = int(effective_extract * self.z_focus_offset)
                z_start = max(0, z_center - z_below)
                z_end = min(z_total, z_start + effective_extract)
                z_start = max(0, z_end - effective_extract)
                z_ranges[exp.name] = (z_start, z_end)
        if self.z_window is not None and z_ranges:
            for name, (z_s, z_e) in z_ranges.items():
                if z_e - z_s < self.z_window:
                    raise ValueError(f"Experiment '{name}': extraction range ({z_e - z_s}) < z_window ({self.z_window}). "
                                     f"Increase z_extraction_window or reduce z_window.")
        self.z_ranges = z_ranges
        if self.reference_pixel_size_xy_um is not None:
            missing = [e.name for e in experiments if e.pixel_size_xy_um is None]
            if missing:
                raise ValueError(f"reference_pixel_size_xy_um set but experiments missing pixel_size_xy_um: {missing}")
        if self.reference_pixel_size_z_um is not None:
            missing = [e.name for e in experiments if e.pixel_size_z_um is None]
            if missing:
                raise ValueError(f"reference_pixel_size_z_um set but experiments missing pixel_size_z_um: {missing}")
        self.scale_factors = self._compute_scale_factors()

    @property
    def experiments(self) -> list:
        return self.collection.experiments

    @property
    def source_channel_labels(self) -> list[str]:
        seen, labels = set(), []
        for exp in self.collection.experiments:
            for ch in exp.channels:
                if ch.marker not in seen:
                    labels.append(ch.marker)
                    seen.add(ch.marker)
        return labels

    def _compute_scale_factors(self) -> dict:
        out = {}
        for exp in self.collection.experiments:
            scale_y = scale_x = scale_z = 1.0
            if self.reference_pixel_size_xy_um is not None and exp.pixel_size_xy_um is not None:
                scale_y = scale_x = self.reference_pixel_size_xy_um / exp.pixel_size_xy_um
            if self.reference_pixel_size_z_um is not None and exp.pixel_size_z_um is not None:
                scale_z = self.reference_pixel_size_z_um / exp.pixel_size_z_um
            out[exp.name] = (scale_z, scale_y, scale_x)
        return out

    @classmethod
    def from_collection(cls, path, **kw):
        raise NotImplementedError("ExperimentRegistry.from_collection (collection YAML) is not built: use from_cell_index")

    @classmethod
    def from_cell_index(cls, cell_index_path, z_window: int | None = None, z_extraction_window: int | None = None,
                        z_focus_offset: float = 0.5, focus_channel: str | None = None,
                        reference_pixel_size_xy_um: float | None = None, reference_pixel_size_z_um: float | None = None):
        """-> (registry, DataFrame): experiments, their channels (``marker`` / ``channel_name`` pairs), wells per perturbation,
        frame interval and pixel sizes derived from the flat parquet; channel names and Z from one FOV per store"""
        df = read_cell_index(cell_index_path)
        if df.empty:
            raise ValueError(f"Cell index is empty: {cell_index_path}")
        channel_names_cache = {}
        for store_path, group in df.groupby("store_path", observed=True):
            first = group.iloc[0]
            pos = open_ome_zarr(f"{store_path}/{first['well']}/{first['fov']}", mode="r")
            channel_names_cache[str(store_path)] = list(pos.channel_names)
        exp_channels, exp_seen = defaultdict(list), defaultdict(set)
        for (exp_name, marker, ch_name), _ in df.groupby(["experiment", "marker", "channel_name"], observed=True):
            exp_name, marker, ch_name = str(exp_name), str(marker), str(ch_name)
            if (ch_name, marker) not in exp_seen[exp_name]:
                exp_channels[exp_name].append(ChannelEntry(name=ch_name, marker=marker))
                exp_seen[exp_name].add((ch_name, marker))
        experiments = []
        for exp_name, exp_group in df.groupby("experiment", observed=True):
            exp_name = str(exp_name)
            store_path = str(exp_group["store_path"].iloc[0])
            perturbation_wells, seen_pairs = defaultdict(list), set()
            for _, row in exp_group[["perturbation", "well"]].drop_duplicates().iterrows():
                cond, well = str(row["perturbation"]), str(row["well"])
                if (cond, well) not in seen_pairs:
                    perturbation_wells[cond].append(well)
                    seen_pairs.add((cond, well))

            def first_of(col, cast, default):
                if col in exp_group.columns:
                    values = exp_group[col].dropna()
                    if not values.empty:
                        return cast(values.iloc[0])
                return default

            if "interval_minutes" not in exp_group.columns or exp_group["interval_minutes"].dropna().empty:
                raise ValueError(f"Experiment '{exp_name}': cell index parquet missing 'interval_minutes'. "
                                 "Rebuild the parquet with `build-cell-index`.")
            experiments.append(ExperimentEntry(
                name=exp_name, data_path=store_path, tracks_path="", channels=exp_channels.get(exp_name, []),
                channel_names=channel_names_cache[store_path], perturbation_wells=dict(perturbation_wells),
                interval_minutes=float(exp_group["interval_minutes"].dropna().iloc[0]), marker=first_of("marker", str, ""),
                organelle=first_of("organelle", str, ""), pixel_size_xy_um=first_of("pixel_size_xy_um", float, None),
                pixel_size_z_um=first_of("pixel_size_z_um", float, None)))
        collection = Collection(name=Path(cell_index_path).stem, description=f"Auto-generated from cell index: {cell_index_path}",
                                experiments=experiments)
        registry = cls(collection=collection, z_window=z_window, z_extraction_window=z_extraction_window,
                       z_focus_offset=z_focus_offset, focus_channel=focus_channel,
                       reference_pixel_size_xy_um=reference_pixel_size_xy_um, reference_pixel_size_z_um=reference_pixel_size_z_um)
        return registry, df

    def subset(self, experiment_names: list[str]) -> "ExperimentRegistry":
        c = self.collection
        sub = Collection(name=c.name, description=c.description, provenance=c.provenance, fov_records=c.fov_records,
                         experiments=[e for e in c.experiments if e.name in experiment_names])
        return ExperimentRegistry(collection=sub, z_window=self.z_window, z_extraction_window=self.z_extraction_window,
                                  z_focus_offset=self.z_focus_offset, focus_channel=self.focus_channel,
                                  reference_pixel_size_xy_um=self.reference_pixel_size_xy_um,
                                  reference_pixel_size_z_um=self.reference_pixel_size_z_um)

    def tau_range_frames(self, experiment_name: str, tau_range_hours: tuple[float, float]) -> tuple[int, int]:
        exp = self.get_experiment(experiment_name)
        min_frames = round(tau_range_hours[0] * 60 / exp.interval_minutes)
        max_frames = round(tau_range_hours[1] * 60 / exp.interval_minutes)
        if min_frames >= max_frames:
            _logger.warning("Experiment '%s': tau_range_hours=%s yields fewer than 2 valid frames (min=%d, max=%d).",
                            experiment_name, tau_range_hours, min_frames, max_frames)
        return (min_frames, max_frames)

    def get_experiment(self, name: str) -> ExperimentEntry:
        try:
            return self._name_map[name]
        except KeyError:
            raise KeyError(f"Experiment '{name}' not found in registry. Available: {list(self._name_map.keys())}")


# ------------------------------------------------------------------------------------------------ index (index.py)
class MultiExperimentIndex:
    """``dynaclr.data.index.MultiExperimentIndex`` over a cell-index parquet (``cell_index_path`` or ``cell_index_df``):
    ``tracks`` (one row per cell observation, border-clamped centres ``y_clamp`` / ``x_clamp``) and ``valid_anchors`` (the rows
    that have a positive under ``positive_cell_source`` / ``positive_match_columns`` / ``tau_range_hours``)."""

    def __init__(self, registry: ExperimentRegistry, yx_patch_size: tuple[int, int], tau_range_hours: tuple[float, float] = (0.5, 2.0),
                 include_wells: list[str] | None = None, exclude_fovs: list[str] | None = None, cell_index_path=None,
                 cell_index_df=None, num_workers: int = 1, positive_cell_source: str = "lookup",
                 positive_match_columns: list[str] | None = None, max_border_shift: int = -1, fit: bool = True,
                 tensorstore_config=None) -> None:
        self.registry, self.yx_patch_size, self.tau_range_hours = registry, yx_patch_size, tau_range_hours
        if max_border_shift < 0:
            max_border_shift = max(yx_patch_size[0] // 4, yx_patch_size[1] // 4)
        self.max_border_shift = max_border_shift
        self.tensorstore_config = tensorstore_config  # accepted and unused: frames are read by this package's OME-Zarr reader
        self._store_cache: dict = {}
        collection_excludes: set = set()
        for exp in registry.experiments:
            collection_excludes.update(exp.exclude_fovs)
        if exclude_fovs is not None:
            all_exclude_fovs = list(collection_excludes | set(exclude_fovs))
        elif collection_excludes:
            all_exclude_fovs = list(collection_excludes)
        else:
            all_exclude_fovs = None
        if cell_index_df is None and cell_index_path is None:
            self._load_all_experiments(include_wells=include_wells, exclude_fovs=all_exclude_fovs, num_workers=num_workers)
        if cell_index_df is not None:
            tracks = self._align_parquet_columns(cell_index_df.copy())
        else:
            tracks = self._align_parquet_columns(read_cell_index(cell_index_path))
        if include_wells is not None:
            tracks = tracks[tracks["well_name"].isin(include_wells)].copy()
        if all_exclude_fovs is not None:
            tracks = tracks[~tracks["fov_name"].isin(all_exclude_fovs)].copy()
        tracks = self._filter_to_registry_experiments(tracks)
        tracks = self._resolve_dims(tracks)
        tracks = self._clamp_borders(tracks)
        self.tracks = tracks.reset_index(drop=True)
        if fit:
            self.valid_anchors = self._compute_valid_anchors(tau_range_hours, positive_cell_source=positive_cell_source,
                                                             positive_match_columns=positive_match_columns)
            if self.valid_anchors.empty and not self.tracks.empty:
                raise ValueError(f"No valid anchors found from {len(self.tracks)} tracks. "
                                 f"positive_cell_source={positive_cell_source!r}, positive_match_columns={positive_match_columns!r}, "
                                 f"tau_range_hours={tau_range_hours}. Check that tracks have matching positives under these settings.")
        else:
            self.valid_anchors = self.tracks

    def _load_all_experiments(self, include_wells, exclude_fovs, num_workers):
        raise NotImplementedError("_load_all_experiments (a cell index built from zarr stores and tracking CSVs) is not built: "
                                  "pass cell_index_path or cell_index_df")

    @staticmethod
    def _reconstruct_lineage(tracks):
        raise NotImplementedError("_reconstruct_lineage is not built: the cell-index parquet carries lineage_id")

    @staticmethod
    def _align_parquet_columns(tracks):
        tracks = tracks.rename(columns={"fov": "fov_name", "well": "well_name"})
        if "fov_name" in tracks.columns and "well_name" in tracks.columns:
            needs_prefix = ~tracks["fov_name"].str.contains("/")
            if needs_prefix.any():
                tracks.loc[needs_prefix, "fov_name"] = tracks.loc[needs_prefix, "well_name"] + "/" + tracks.loc[needs_prefix, "fov_name"]
        if "microscope" not in tracks.columns:
            tracks["microscope"] = ""
        for col in ("fov_name", "well_name"):
            if col in tracks.columns and tracks[col].dtype == object:
                tracks[col] = tracks[col].astype("category")
        return tracks

    def _filter_to_registry_experiments(self, tracks):
        return tracks[tracks["experiment"].isin({exp.name for exp in self.registry.experiments})].copy()

    def _resolve_dims(self, tracks):
        import pandas as pd

        if tracks.empty:
            tracks["_img_height"], tracks["_img_width"] = pd.Series(dtype=int), pd.Series(dtype=int)
            return tracks
        if "Y_shape" in tracks.columns and "X_shape" in tracks.columns and tracks["Y_shape"].notna().all() \
                and tracks["X_shape"].notna().all():
            tracks["_img_height"], tracks["_img_width"] = tracks["Y_shape"], tracks["X_shape"]
            return tracks
        _logger.warning("Parquet missing Y_shape/X_shape columns. Falling back to opening zarr stores for image dimensions.")
        dim_lookup = {}
        for (store_path, well_name, fov_name), _group in tracks.groupby(["store_path", "well_name", "fov_name"], observed=True):
            if store_path not in self._store_cache:
                self._store_cache[store_path] = open_ome_zarr(store_path, mode="r")
            image = self._store_cache[store_path][fov_name if "/" in fov_name else f"{well_name}/{fov_name}"]["0"]
            dim_lookup[(store_path, fov_name)] = (image.height, image.width)
        tracks["_img_height"] = [dim_lookup[(sp, fn)][0] for sp, fn in zip(tracks["store_path"], tracks["fov_name"])]
        tracks["_img_width"] = [dim_lookup[(sp, fn)][1] for sp, fn in zip(tracks["store_path"], tracks["fov_name"])]
        return tracks

    def _clamp_borders(self, tracks):
        if tracks.empty:
            return tracks
        y_half, x_half = self.yx_patch_size[0] // 2, self.yx_patch_size[1] // 2
        max_shift = self.max_border_shift
        valid = (tracks["y"] >= 0) & (tracks["y"] < tracks["_img_height"]) & (tracks["x"] >= 0) & (tracks["x"] < tracks["_img_width"])
        tracks = tracks[valid].copy()
        if max_shift > 0:
            tracks["y_clamp"] = np.clip(tracks["y"].to_numpy(), y_half, (tracks["_img_height"] - y_half).to_numpy())
            tracks["x_clamp"] = np.clip(tracks["x"].to_numpy(), x_half, (tracks["_img_width"] - x_half).to_numpy())
            y_shift = np.abs(tracks["y_clamp"].to_numpy() - tracks["y"].to_numpy())
            x_shift = np.abs(tracks["x_clamp"].to_numpy() - tracks["x"].to_numpy())
            tracks = tracks[(y_shift <= max_shift) & (x_shift <= max_shift)].copy()
        else:
            in_bounds = ((tracks["y"] >= y_half) & (tracks["y"] <= tracks["_img_height"] - y_half)
                         & (tracks["x"] >= x_half) & (tracks["x"] <= tracks["_img_width"] - x_half))
            tracks = tracks[in_bounds].copy()
            tracks["y_clamp"], tracks["x_clamp"] = tracks["y"], tracks["x"]
        return tracks.drop(columns=["_img_height", "_img_width"])

    def _compute_valid_anchors(self, tau_range_hours, positive_cell_source: str = "lookup", positive_match_columns=None):
        import pandas as pd

        if self.tracks.empty:
            return self.tracks.copy()
        if positive_cell_source == "self":
            return self.tracks.reset_index(drop=True)
        if positive_match_columns is not None and "lineage_id" not in positive_match_columns:
            group_sizes = self.tracks.groupby(list(positive_match_columns), observed=True).transform("size")
            return self.tracks[group_sizes >= 2].reset_index(drop=True)
        # temporal: (lineage, [marker,] t + tau) must exist for some tau of the experiment's window; the marker is part of the
        # key because the dataset restricts candidates to the anchor's marker in a flat parquet
        key_cols = ["lineage_id", "marker", "t"] if "marker" in self.tracks.columns else ["lineage_id", "t"]
        valid_mask = np.zeros(len(self.tracks), dtype=bool)
        for exp in self.registry.experiments:
            min_f, max_f = self.registry.tau_range_frames(exp.name, tau_range_hours)
            exp_mask = self.tracks["experiment"] == exp.name
            exp_df = self.tracks.loc[exp_mask, key_cols]
            if exp_df.empty:
                continue
            existing = exp_df.drop_duplicates()
            existing_mi = pd.MultiIndex.from_frame(existing)
            found_any = np.zeros(len(existing), dtype=bool)
            t_vals = existing["t"].to_numpy()
            non_t_arrays = [existing[c].to_numpy() for c in key_cols if c != "t"]
            for tau in (tau for tau in range(min_f, max_f + 1) if tau != 0):
                found_any |= pd.MultiIndex.from_arrays(non_t_arrays + [t_vals + tau]).isin(existing_mi)
            valid_pairs_mi = pd.MultiIndex.from_frame(existing[found_any])
            valid_mask[exp_mask.to_numpy()] = pd.MultiIndex.from_frame(exp_df).isin(valid_pairs_mi)
        return self.tracks[valid_mask].reset_index(drop=True)

    @property
    def experiment_groups(self) -> dict:
        return {name: group.index.to_numpy() for name, group in self.tracks.groupby("experiment", observed=True)}

    @property
    def condition_groups(self) -> dict:
        return {name: group.index.to_numpy() for name, group in self.tracks.groupby("perturbation", observed=True)}

    def clone_with_subset(self, tracks_subset, positive_cell_source: str = "lookup", positive_match_columns=None,
                          max_border_shift: int = -1, precomputed_valid_anchors=None) -> "MultiExperimentIndex":
        clone = object.__new__(MultiExperimentIndex)
        clone.registry, clone.yx_patch_size, clone.tau_range_hours = self.registry, self.yx_patch_size, self.tau_range_hours
        clone._store_cache, clone.tensorstore_config = self._store_cache, self.tensorstore_config
        clone.max_border_shift = self.max_border_shift if max_border_shift < 0 else max_border_shift
        clone.tracks = tracks_subset.reset_index(drop=True)
        if precomputed_valid_anchors is not None:
            clone.valid_anchors = precomputed_valid_anchors.reset_index(drop=True)
        else:
            clone.valid_anchors = clone._compute_valid_anchors(tau_range_hours=self.tau_range_hours,
                                                               positive_cell_source=positive_cell_source,
                                                               positive_match_columns=positive_match_columns)
        if clone.valid_anchors.empty and not clone.tracks.empty:
            raise ValueError(f"No valid anchors found from {len(clone.tracks)} tracks in subset. "
                             f"positive_cell_source={positive_cell_source!r}, positive_match_columns={positive_match_columns!r}. "
                             "Check that the subset has matching positives under these settings.")
        return clone

    def summary(self) -> str:
        lines = [f"MultiExperimentIndex: {len(self.registry.experiments)} experiments, {len(self.tracks)} total observations, "
                 f"{len(self.valid_anchors)} valid anchors"]
        for exp in self.registry.experiments:
            exp_tracks = self.tracks[self.tracks["experiment"] == exp.name]
            exp_anchors = self.valid_anchors[self.valid_anchors["experiment"] == exp.name]
            cond_counts = exp_tracks.groupby("perturbation", observed=True).size()
            cond_str = ", ".join(f"{c}({n})" for c, n in cond_counts.items())
            lines.append(f"  {exp.name}: {len(exp_tracks)} observations, {len(exp_anchors)} anchors, conditions: {cond_str}")
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ dataset (dataset.py)
_META_COLUMNS = ["experiment", "perturbation", "microscope", "fov_name", "store_path", "global_track_id", "t",
                 "hours_post_perturbation", "lineage_id", "marker", "y_clamp", "x_clamp"]
_HOT_COLUMNS = {"channel_name", "experiment", "lineage_id", "t", "marker", "store_path", "fov_name", "y_clamp", "x_clamp",
                "norm_mean", "norm_std", "norm_median", "norm_iqr"}
_PREDICT_INDEX_COLUMNS = list(ULTRACK_INDEX_COLUMNS) + ["experiment", "marker", "perturbation", "hours_post_perturbation",
                                                        "organelle", "well", "microscope"]


@dataclass(frozen=True)
class PatchBox:
    """what ``_slice_patch`` decides for one row: the frame, the channels, the native box and the target size"""

    key: tuple            # (store_path, fov_name, t)
    experiment: str
    channels: tuple       # zarr channel indices
    z_start: int
    z_count: int
    y_start: int
    y_count: int
    x_start: int
    x_count: int
    scale: tuple          # (scale_z, scale_y, scale_x)
    target: tuple         # (Zt, Yt, Xt)

    @property
    def native(self) -> tuple:
        return (self.z_count, self.y_count, self.x_count)


class MultiExperimentTripletDataset(Dataset):
    """``dynaclr.data.dataset.MultiExperimentTripletDataset``: anchors and positives over a ``MultiExperimentIndex``; keywords,
    defaults, exceptions and batch keys are the reference's.  ``__getitems__(indices)`` forms a batch: float32
    ``[B, C, Zt, Yt, Xt]`` tensors on ``device`` from ONE ``patch_gather_scaled`` launch for anchor and positive together, the
    per-sample ``*_norm_meta`` and ``*_meta`` lists (fit), or ``anchor`` and ``index`` (predict).  ``device``: where the batch is made
    (default: the current HIP device, else the CPU, where ``host_gather`` cuts through the same tables);
    ``device_cache_bytes``: the frame budget (``None``: half of the free device memory at construction)."""

    def __init__(self, index: MultiExperimentIndex, fit: bool = True, tau_range_hours: tuple[float, float] = (0.5, 2.0),
                 tau_decay_rate: float = 2.0, return_negative: bool = False, channels_per_sample: int | list[str] | None = None,
                 positive_cell_source: str = "lookup", positive_match_columns: list[str] | None = None,
                 positive_channel_source: str = "same", label_columns: dict[str, str] | None = None, device=None,
                 device_cache_bytes: int | None = None) -> None:
        if return_negative:
            raise NotImplementedError("return_negative is not built (the reference reserves it too: NT-Xent uses in-batch negatives)")
        self.index, self.fit = index, fit
        self.tau_range_hours, self.tau_decay_rate, self.return_negative = tau_range_hours, tau_decay_rate, return_negative
        if channels_per_sample is None:
            self._channel_mode = "all"
            va = index.valid_anchors
            if va["cell_id"].duplicated().any():  # flat parquet (one row per cell and channel): every row reads all channels
                index.valid_anchors = va.drop_duplicates(subset="cell_id").reset_index(drop=True)
        elif isinstance(channels_per_sample, int):
            if channels_per_sample != 1:
                raise ValueError(f"channels_per_sample as int must be 1, got {channels_per_sample}. "
                                 "Use a list of labels for multiple specific channels.")
            self._channel_mode = "from_index"
        elif isinstance(channels_per_sample, list):
            self._channel_mode = "fixed"
            self._fixed_channel_names = channels_per_sample
        else:
            raise TypeError(f"channels_per_sample must be int, list[str], or None, got {type(channels_per_sample)}")
        self.channels_per_sample = channels_per_sample
        self.positive_cell_source = positive_cell_source
        self.positive_match_columns = positive_match_columns if positive_match_columns is not None else ["lineage_id"]
        self.positive_channel_source = positive_channel_source
        self._label_encoders: dict = {}
        if label_columns:
            for batch_key, col in label_columns.items():
                unique_vals = sorted(index.valid_anchors[col].dropna().unique())
                self._label_encoders[batch_key] = (col, {v: i for i, v in enumerate(unique_vals)})
        self._rng = np.random.default_rng()
        self._store_cache, self._position_cache, self._image_cache, self._norm_meta_cache = {}, {}, {}, {}
        self._table_cache, self._channel_tables = {}, {}  # axis tables by (start, count, target, rescale); channel tables by tuple
        if self.fit:
            self._build_match_lookup()
        self._build_anchor_cache()
        self.device = default_device(device)
        self.cache = None
        if self.device.type == "cuda":
            if device_cache_bytes is None:
                device_cache_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
            self.cache = FrameCache(self._load_frame, self._frame_nbytes, self.device, int(device_cache_bytes))
        self._cutter = PatchCutter(self.device, self.cache, self._load_frame)

    # ------------------------------------------------------------------ lookups (dataset.py:265-382)
    def _build_match_lookup(self) -> None:
        if self.positive_cell_source == "self":
            return
        tracks = self.index.tracks
        if "lineage_id" in self.positive_match_columns:
            grouped = tracks.groupby(["experiment", "lineage_id", "t"], observed=True).indices
            self._lineage_timepoints = defaultdict(lambda: defaultdict(list))
            for (exp, lid, t), row_indices in grouped.items():
                self._lineage_timepoints[(str(exp), str(lid))][int(t)] = row_indices.tolist()
        else:
            grouped = tracks.groupby(self.positive_match_columns, observed=True).indices
            self._match_lookup = {(k if isinstance(k, tuple) else (k,)): v for k, v in grouped.items()}

    def _build_anchor_cache(self) -> None:
        import pandas as pd

        def cache_columns(df, columns):
            out = {}
            for col in columns:
                if col not in df.columns:
                    continue
                s = df[col]
                out[col] = s.astype("category").array if s.dtype == object or pd.api.types.is_string_dtype(s) else s.to_numpy()
            return out

        hot = set(_HOT_COLUMNS)
        if self.positive_match_columns:
            hot.update(self.positive_match_columns)
        for col, _encoder in self._label_encoders.values():
            hot.add(col)
        self._va_arrays = cache_columns(self.index.valid_anchors, sorted(hot))
        self._tr_arrays = cache_columns(self.index.tracks, sorted(hot))
        self._tau_range_frames_cache = {}
        for name, exp in self.index.registry._name_map.items():
            if getattr(exp, "interval_minutes", 0):
                self._tau_range_frames_cache[name] = self.index.registry.tau_range_frames(name, self.tau_range_hours)

    def __len__(self) -> int:
        return len(self.index.valid_anchors)

    def __getitem__(self, idx: int) -> None:
        raise NotImplementedError("MultiExperimentTripletDataset only supports batched access via __getitems__. "
                                  "Use a batch sampler with collate_fn=lambda x: x.")

    # ------------------------------------------------------------------ batches (dataset.py:398-474)
    def __getitems__(self, indices: list[int]) -> dict:
        anchor_rows = self.index.valid_anchors.iloc[indices]
        if self._channel_mode == "from_index":
            chan_arr = self._va_arrays["channel_name"]
            forced = [[chan_arr[i]] for i in indices]
        elif self._channel_mode == "fixed":
            forced = [self._fixed_channel_names] * len(indices)
        else:
            forced = None
        boxes, anchor_norms = self._slice_boxes(self._va_arrays, indices, forced)
        B = len(boxes)
        sample = {"anchor_norm_meta": anchor_norms, "anchor_meta": self._extract_meta(anchor_rows)}
        if self.positive_cell_source == "self" or not self.fit:
            (sample["anchor_norm_meta"],) = self._norms_on_device(anchor_norms)
        lookup = self.fit and self.positive_cell_source != "self"
        if lookup:
            pos_track_indices = self._sample_positive_indices(anchor_positions=indices)
            if self._channel_mode == "from_index":
                tr_chan_arr = self._tr_arrays["channel_name"]
                pos_forced = [[tr_chan_arr[i]] for i in pos_track_indices]
            else:
                pos_forced = forced
            positive_boxes, positive_norms = self._slice_boxes(self._tr_arrays, pos_track_indices, pos_forced)
            boxes = boxes + positive_boxes
        patches = self._cut(boxes)  # anchor and positive: one descriptor table, one begin_batch, one launch
        sample["anchor"] = patches[:B]
        if lookup:
            sample["anchor_norm_meta"], positive_norms = self._norms_on_device(anchor_norms, positive_norms)
            sample["positive"] = patches[B:]
            sample["positive_norm_meta"] = positive_norms
            sample["positive_meta"] = self._extract_meta(self.index.tracks.iloc[pos_track_indices].reset_index(drop=True))
        elif self.fit:
            # SimCLR: the positive is the anchor's patch; the clone gives the augmentations a buffer of their own
            sample["positive"] = sample["anchor"].clone()
            sample["positive_norm_meta"] = sample["anchor_norm_meta"]
            sample["positive_meta"] = sample["anchor_meta"]
        else:
            present = [c for c in _PREDICT_INDEX_COLUMNS if c in anchor_rows.columns]
            col_arrays = {c: anchor_rows[c].to_numpy() for c in present}
            sample["index"] = [{c: col_arrays[c][i] for c in present} for i in range(len(anchor_rows))]
        return sample

    def _norms_on_device(self, *norm_lists):
        """the statistics of a batch's norm-meta trees as views of ONE tensor uploaded once (the trees are born on the host, one
        0-d tensor per statistic, as the reference's are; moved one by one they would cost a copy each)"""
        if self.device.type != "cuda":
            return norm_lists
        leaves = []

        def collect(tree):
            if isinstance(tree, dict):
                for v in tree.values():
                    collect(v)
            elif torch.is_tensor(tree):
                leaves.append(tree)

        for trees in norm_lists:
            for tree in trees:
                collect(tree)
        if not leaves:
            return norm_lists
        moved = iter(torch.stack(leaves).pin_memory().to(self.device, non_blocking=True).unbind(0))

        def rebuild(tree):
            if isinstance(tree, dict):
                return {k: rebuild(v) for k, v in tree.items()}
            return next(moved) if torch.is_tensor(tree) else tree

        return tuple([rebuild(tree) for tree in trees] for trees in norm_lists)

    def _extract_meta(self, rows) -> list[dict]:
        cols = [c for c in _META_COLUMNS if c in rows.columns]
        records = rows[cols].to_dict(orient="records")
        if self._label_encoders:
            label_arrays = {batch_key: (encoder, rows[col].to_numpy() if col in rows.columns else None)
                            for batch_key, (col, encoder) in self._label_encoders.items()}
            for i in range(len(records)):
                labels = {}
                for batch_key, (encoder, arr) in label_arrays.items():
                    if arr is None:
                        continue
                    val = arr[i]
                    if val is not None and val in encoder:
                        labels[batch_key] = encoder[val]
                records[i]["labels"] = labels
        return records

    # ------------------------------------------------------------------ positives (dataset.py:515-634)
    def _sample_positive_indices(self, anchor_positions: list[int]) -> np.ndarray:
        if "lineage_id" in self.positive_match_columns:
            return self._sample_positive_indices_temporal(anchor_positions)
        va_col_arrs = [self._va_arrays[c] for c in self.positive_match_columns]
        out = np.empty(len(anchor_positions), dtype=np.int64)
        for i, ai in enumerate(anchor_positions):
            key = tuple(arr[ai] for arr in va_col_arrs)
            cands = self._match_lookup.get(key)
            if cands is None or len(cands) == 0:
                raise RuntimeError(f"No positive found for anchor at position {ai} key={key}. "
                                   "This anchor should have been filtered out by valid_anchors.")
            out[i] = cands[self._rng.integers(len(cands))]
        return out

    def _sample_positive_indices_temporal(self, anchor_positions: list[int]) -> np.ndarray:
        exp_arr, lid_arr, t_arr = self._va_arrays["experiment"], self._va_arrays["lineage_id"], self._va_arrays["t"]
        marker_filter = self._channel_mode == "from_index"  # flat parquet: candidates of the anchor's marker
        if marker_filter:
            anchor_marker_arr, tr_marker_arr = self._va_arrays["marker"], self._tr_arrays["marker"]
        out = np.empty(len(anchor_positions), dtype=np.int64)
        for i, ai in enumerate(anchor_positions):
            exp_name, lineage_id, anchor_t = str(exp_arr[ai]), str(lid_arr[ai]), int(t_arr[ai])
            tau_min, tau_max = self._tau_range_frames_cache[exp_name]
            timepoints = self._lineage_timepoints.get((exp_name, lineage_id))
            chosen = None
            if timepoints is not None:
                chosen = _pick_temporal_candidate(timepoints, anchor_t, tau_min, tau_max, self.tau_decay_rate, self._rng,
                                                  tr_marker_arr if marker_filter else None,
                                                  anchor_marker_arr[ai] if marker_filter else None)
            if chosen is None:
                raise RuntimeError(f"No positive found for anchor at position {ai} (experiment={exp_name}, "
                                   f"lineage_id={lineage_id}, t={anchor_t}). This anchor should have been filtered out by valid_anchors.")
            out[i] = chosen
        return out

    # ------------------------------------------------------------------ frames
    def _get_position(self, store_path: str, fov_name: str):
        key = (store_path, fov_name)  # the same FOV name appears in several stores
        if key not in self._position_cache:
            if store_path not in self._store_cache:
                self._store_cache[store_path] = open_ome_zarr(store_path, mode="r")
            self._position_cache[key] = self._store_cache[store_path][fov_name]
        return self._position_cache[key]

    def _image(self, store_path: str, fov_name: str):
        key = (store_path, fov_name)
        image = self._image_cache.get(key)
        if image is None:
            image = self._image_cache[key] = self._get_position(store_path, fov_name)["0"]
            check_storage_dtype(image.dtype, f"{store_path}/{fov_name}")
        return image

    def _frame_nbytes(self, key) -> int:
        image = self._image(key[0], key[1])
        return int(np.prod(image.shape[1:])) * np.dtype(image.dtype).itemsize

    def _load_frame(self, key) -> np.ndarray:
        """the (C, Z, H, W) block of time point ``t`` of a FOV, every channel and plane: rows of one frame name different channels"""
        image = self._image(key[0], key[1])
        return image.oindex[int(key[2]), list(range(image.channels)), slice(0, image.slices)][0]

    # ------------------------------------------------------------------ boxes and norm meta (dataset.py:694-854)
    def _build_norm_meta(self, arrays: dict, idx: int, forced_channel_names):
        norm_mean_arr = arrays.get("norm_mean")
        if norm_mean_arr is not None:
            norm_mean = norm_mean_arr[idx]
            if norm_mean is not None and not (isinstance(norm_mean, (float, np.floating)) and np.isnan(norm_mean)):
                tp_stats = {"mean": torch.tensor(norm_mean, dtype=torch.float32),
                            "std": torch.tensor(arrays["norm_std"][idx], dtype=torch.float32),
                            "median": torch.tensor(arrays["norm_median"][idx], dtype=torch.float32),
                            "iqr": torch.tensor(arrays["norm_iqr"][idx], dtype=torch.float32)}
                if self._channel_mode == "from_index":
                    return {"channel_0": {"timepoint_statistics": tp_stats}}
                ch_arr = arrays.get("channel_name")
                return {(ch_arr[idx] if ch_arr is not None else "channel_0"): {"timepoint_statistics": tp_stats}}
        store_path, fov_name, t = arrays["store_path"][idx], arrays["fov_name"][idx], arrays["t"][idx]
        cache_key = (store_path, fov_name)
        if cache_key not in self._norm_meta_cache:
            self._norm_meta_cache[cache_key] = read_norm_meta(self._get_position(store_path, fov_name))
        cached = self._norm_meta_cache[cache_key]
        if cached is None:
            return None
        raw = {}
        for ch, ch_meta in cached.items():
            raw[ch] = {level: (stats.get(str(t)) if level == "timepoint_statistics" and isinstance(stats, dict) else stats)
                       for level, stats in ch_meta.items()}
        if forced_channel_names is not None and self._channel_mode == "from_index":
            ch = forced_channel_names[0]
            return {"channel_0": raw[ch]} if ch in raw else None
        if forced_channel_names is not None and self._channel_mode == "fixed":
            return {name: raw[name] for name in forced_channel_names if name in raw} or None
        return raw

    def _slice_patch(self, arrays: dict, idx: int, forced_channel_names=None) -> tuple[PatchBox, dict | None]:
        """dataset.py:768-854 up to the read: the frame, the channel indices, the native box (``round`` of the scaled half sizes
        around ``y_clamp`` / ``x_clamp``; ``round`` of the scaled Z window around the centre of the experiment's Z range) and the
        uniform target size (``z_extraction_window`` as Z)"""
        store_path, fov_name, exp_name = arrays["store_path"][idx], arrays["fov_name"][idx], arrays["experiment"][idx]
        registry, yx = self.index.registry, self.index.yx_patch_size
        t, y_center, x_center = int(arrays["t"][idx]), int(arrays["y_clamp"][idx]), int(arrays["x_clamp"][idx])
        scale_z, scale_y, scale_x = registry.scale_factors[exp_name]
        y_half, x_half = round((yx[0] // 2) * scale_y), round((yx[1] // 2) * scale_x)
        exp = registry._name_map[exp_name]
        names = forced_channel_names if forced_channel_names is not None else exp.channel_names
        channel_indices = tuple(exp.channel_names.index(name) for name in names)
        z_start_base, z_end_base = registry.z_ranges[exp_name]
        z_window_size = z_end_base - z_start_base
        z_count = round(z_window_size * scale_z)
        z_start = (z_start_base + z_end_base) // 2 - z_count // 2
        box = PatchBox(key=(str(store_path), str(fov_name), t), experiment=str(exp_name), channels=channel_indices,
                       z_start=z_start, z_count=z_count, y_start=y_center - y_half, y_count=2 * y_half,
                       x_start=x_center - x_half, x_count=2 * x_half, scale=(scale_z, scale_y, scale_x),
                       target=(registry.z_extraction_window or z_window_size, yx[0], yx[1]))
        return box, self._build_norm_meta(arrays, idx, forced_channel_names)

    def _slice_boxes(self, arrays: dict, indices, forced_channel_names=None) -> tuple[list, list]:
        boxes, norms = [], []
        for i, idx in enumerate(indices):
            box, norm = self._slice_patch(arrays, int(idx), forced_channel_names[i] if forced_channel_names is not None else None)
            boxes.append(box)
            norms.append(norm)
        return boxes, norms

    def _axis_table(self, start: int, count: int, target: int, rescale: bool) -> np.ndarray:
        """absolute source positions of one axis of a box: the native positions as they are, or ``nearest_exact_index`` of them;
        one array object per (start, count, target, rescale), so patches of one experiment share their Z tables in the launch"""
        key = (start, count, target, rescale)
        table = self._table_cache.get(key)
        if table is None:
            if len(self._table_cache) > 65536:
                self._table_cache.clear()
            if count <= 0:
                raise ValueError(f"a native box of {count} elements from {start}: nothing to read")
            table = start + (nearest_exact_index(count, target) if rescale else np.arange(count, dtype=np.int64))
            self._table_cache[key] = table
        return table

    def _tables(self, box: PatchBox) -> tuple:
        """(channel, z, y, x) tables of a box.  ``_rescale_patch`` leaves a patch alone when all three scales are 1.0 and resamples
        all three axes to the target otherwise."""
        rescale = box.scale != (1.0, 1.0, 1.0)
        chan = self._channel_tables.get(box.channels)
        if chan is None:
            chan = self._channel_tables[box.channels] = np.asarray(box.channels, dtype=np.int64)
        return (chan, self._axis_table(box.z_start, box.z_count, box.target[0], rescale),
                self._axis_table(box.y_start, box.y_count, box.target[1], rescale),
                self._axis_table(box.x_start, box.x_count, box.target[2], rescale))

    def _cut(self, boxes: list) -> Tensor:
        """float32 (n, C, Zt, Yt, Xt) on ``self.device``: one launch over resident frames and a packed block of host-gathered patches
        (one launch per storage dtype where the batch spans stores of different dtypes; the frame cache is asked ONCE for the
        whole batch, so no launch of the batch loses a frame to another's)"""
        tables = [self._tables(b) for b in boxes]
        shapes = {tuple(len(t) for t in ts[1:]) for ts in tables}
        if len(shapes) > 1:  # unscaled boxes keep their native size: torch.stack of the reference fails the same way
            raise RuntimeError(f"stack expects each tensor to be equal size, but patches of one batch are {sorted(shapes)}")
        channel_counts = {len(ts[0]) for ts in tables}
        if len(channel_counts) > 1:
            raise RuntimeError(f"Batch mixes samples with different channel counts: {sorted(channel_counts)}. "
                               "This happens with channels_per_sample=None across experiments that have "
                               "different channel counts. Set channels_per_sample=1 (bag-of-channels) "
                               "or channels_per_sample=[...] (fixed channel list).")
        C, size = channel_counts.pop(), shapes.pop()
        return self._cutter.cut(boxes, [b.key for b in boxes], tables,
                                host_patch=lambda frame, b: host_gather(frame, *self._tables(b)),
                                plain=lambda: tuple(np.arange(s, dtype=np.int64) for s in (C, *size)),
                                launch=lambda sources, ts: ops.patch_gather_scaled(sources, *zip(*ts)),
                                kinds=[np.dtype(self._image(b.key[0], b.key[1]).dtype) for b in boxes])


# ------------------------------------------------------------------------------------------------ module (datamodule.py)
class MultiExperimentDataModule(_DMBase):
    """``dynaclr.data.datamodule.MultiExperimentDataModule``: every constructor keyword of the reference.  ``num_workers``,
    ``pin_memory``, ``prefetch_factor``, ``buffer_size``, ``cache_pool_bytes``, ``recheck_cached_data`` and ``file_io_concurrency`` are
    accepted and unused: batches are formed on the device by the calling thread.  ``device_cache_bytes`` (beyond the
    reference): bytes of device memory for resident frames, per dataset; ``None`` = half of the free device memory at ``setup``."""

    def __init__(self, cell_index_path: str, z_window: int, z_extraction_window: int | None = None, z_focus_offset: float = 0.5,
                 yx_patch_size: tuple[int, int] = (192, 192), final_yx_patch_size: tuple[int, int] = (160, 160),
                 val_experiments: list[str] | None = None, split_ratio: float = 0.8, tau_range: tuple[float, float] = (0.5, 2.0),
                 tau_decay_rate: float = 2.0, batch_size: int = 128, num_workers: int = 4,
                 batch_group_by: str | list[str] | None = None, stratify_by: str | list[str] | None = "perturbation",
                 leaky: float = 0.0, temporal_enrichment: bool = False, temporal_window_hours: float = 2.0,
                 temporal_global_fraction: float = 0.3, group_weights: dict[str, float] | None = None,
                 channels_per_sample: int | list[str] | None = None, channel_dropout_channels: list[int] | None = None,
                 channel_dropout_prob: float = 0.0, normalizations: list | None = None, augmentations: list | None = None,
                 cache_pool_bytes: int = 500_000_000, recheck_cached_data=None, file_io_concurrency: int | None = None,
                 seed: int = 0, include_wells: list[str] | None = None, exclude_fovs: list[str] | None = None,
                 focus_channel: str | None = None, reference_pixel_size_xy_um: float | None = None,
                 reference_pixel_size_z_um: float | None = None, positive_cell_source: str = "lookup",
                 positive_match_columns: list[str] | None = None, positive_channel_source: str = "same",
                 label_columns: dict[str, str] | None = None, max_border_shift: int = -1, shuffle_val: bool = False,
                 pin_memory: bool = True, prefetch_factor: int | None = None, buffer_size: int = 4,
                 device_cache_bytes: int | None = None) -> None:
        if _DMBase is not object:  # pragma: no cover
            super().__init__()
        self.cell_index_path, self.z_window, self.z_extraction_window = cell_index_path, z_window, z_extraction_window
        self.z_focus_offset = z_focus_offset
        self.yx_patch_size, self.final_yx_patch_size = tuple(yx_patch_size), tuple(final_yx_patch_size)
        self.val_experiments = val_experiments if val_experiments is not None else []
        self.split_ratio, self.tau_range, self.tau_decay_rate = split_ratio, tuple(tau_range), tau_decay_rate
        self.batch_size, self.num_workers = batch_size, num_workers
        self.batch_group_by = [batch_group_by] if isinstance(batch_group_by, str) else batch_group_by
        self.stratify_by, self.leaky, self.temporal_enrichment = stratify_by, leaky, temporal_enrichment
        self.temporal_window_hours, self.temporal_global_fraction = temporal_window_hours, temporal_global_fraction
        self.group_weights, self.channels_per_sample = group_weights, channels_per_sample
        self.channel_dropout_channels = channel_dropout_channels if channel_dropout_channels is not None else [1]
        self.channel_dropout_prob = channel_dropout_prob
        self.normalizations = normalizations if normalizations is not None else []
        self.augmentations = augmentations if augmentations is not None else []
        self.cache_pool_bytes, self.recheck_cached_data, self.file_io_concurrency = cache_pool_bytes, recheck_cached_data, file_io_concurrency
        self.seed, self.include_wells, self.exclude_fovs, self.focus_channel = seed, include_wells, exclude_fovs, focus_channel
        self.reference_pixel_size_xy_um, self.reference_pixel_size_z_um = reference_pixel_size_xy_um, reference_pixel_size_z_um
        self.positive_cell_source, self.positive_match_columns = positive_cell_source, positive_match_columns
        self.positive_channel_source, self.label_columns = positive_channel_source, label_columns
        self.max_border_shift, self.shuffle_val = max_border_shift, shuffle_val
        self.pin_memory, self.prefetch_factor, self.buffer_size = pin_memory, prefetch_factor, buffer_size
        self.device_cache_bytes = device_cache_bytes
        self.channel_dropout = ChannelDropout(channels=self.channel_dropout_channels, p=self.channel_dropout_prob)
        self.train_dataset = self.val_dataset = self.predict_dataset = None
        self.trainer = None
        self.device = None  # None: the current HIP device, else the CPU (MultiExperimentTripletDataset)

    def prepare_data(self):
        pass

    # ------------------------------------------------------------------ setup (datamodule.py:276-605)
    def _registry(self):
        return ExperimentRegistry.from_cell_index(
            self.cell_index_path, z_window=self.z_window, z_extraction_window=self.z_extraction_window,
            z_focus_offset=self.z_focus_offset, focus_channel=self.focus_channel,
            reference_pixel_size_xy_um=self.reference_pixel_size_xy_um, reference_pixel_size_z_um=self.reference_pixel_size_z_um)

    def _index_kw(self, cell_index_df) -> dict:
        return dict(yx_patch_size=self.yx_patch_size, tau_range_hours=self.tau_range, include_wells=self.include_wells,
                    exclude_fovs=self.exclude_fovs, cell_index_df=cell_index_df, positive_cell_source=self.positive_cell_source,
                    positive_match_columns=self.positive_match_columns)

    def _dataset(self, index: MultiExperimentIndex, fit: bool) -> MultiExperimentTripletDataset:
        return MultiExperimentTripletDataset(
            index=index, fit=fit, tau_range_hours=self.tau_range, tau_decay_rate=self.tau_decay_rate,
            channels_per_sample=self.channels_per_sample, positive_cell_source=self.positive_cell_source,
            positive_match_columns=self.positive_match_columns, positive_channel_source=self.positive_channel_source,
            label_columns=self.label_columns, device=self.device, device_cache_bytes=self.device_cache_bytes)

    def _resolve_channel_names(self, registry: ExperimentRegistry) -> None:
        if self.channels_per_sample is None:
            self._channel_names = registry.source_channel_labels
        elif isinstance(self.channels_per_sample, int):
            self._channel_names = [f"channel_{i}" for i in range(self.channels_per_sample)]
        else:
            self._channel_names = list(self.channels_per_sample)

    def setup(self, stage: str | None = None) -> None:
        if stage == "fit" or stage is None:
            registry, cell_index_df = self._registry()
            if self.val_experiments:
                self._setup_experiment_split(registry, cell_index_df)
            else:
                self._setup_fov_split(registry, cell_index_df)
            self._resolve_channel_names(registry)
            self._augmentation_transform = Compose(self.normalizations + self.augmentations + [self._train_final_crop()])
        elif stage == "predict":
            self._setup_predict()

    def _setup_predict(self) -> None:
        registry, cell_index_df = self._registry()
        self._resolve_channel_names(registry)
        self.predict_dataset = self._dataset(MultiExperimentIndex(registry=registry, fit=False, **self._index_kw(cell_index_df)), fit=False)
        # predict: normalisations and the final crop; the Z reduction stays, the 2-D models need it
        z_reduction = [t for t in self.augmentations if type(t).__name__ == "BatchedChannelWiseZReductiond"]
        self._predict_transform = Compose(self.normalizations + z_reduction + [self._train_final_crop()])

    def _setup_experiment_split(self, registry: ExperimentRegistry, cell_index_df) -> None:
        train_names = [e.name for e in registry.experiments if e.name not in self.val_experiments]
        val_names = [e.name for e in registry.experiments if e.name in self.val_experiments]
        if not train_names:
            raise ValueError("No training experiments remaining after splitting. "
                             f"val_experiments={self.val_experiments} covers all experiments.")
        if not val_names:
            _logger.warning("No validation experiments found. val_experiments=%s not present in registry.", self.val_experiments)
        kw = dict(max_border_shift=self.max_border_shift, **self._index_kw(cell_index_df))
        self.train_dataset = self._dataset(MultiExperimentIndex(registry=registry.subset(train_names), **kw), fit=True)
        if val_names:
            self.val_dataset = self._dataset(MultiExperimentIndex(registry=registry.subset(val_names), **kw), fit=True)

    def _setup_fov_split(self, registry: ExperimentRegistry, cell_index_df) -> None:
        """FOVs of every experiment split by ``split_ratio`` with ``numpy.random.default_rng(seed)``, keyed (experiment, FOV)"""
        import pandas as pd

        full_index = MultiExperimentIndex(registry=registry, **self._index_kw(cell_index_df))
        rng = np.random.default_rng(self.seed)
        train_fovs_per_exp = {}
        for exp_name, group in full_index.tracks.groupby("experiment", observed=True):
            fovs = sorted(group["fov_name"].unique())
            n_train = max(1, int(len(fovs) * self.split_ratio))
            rng.shuffle(fovs)
            train_fovs_per_exp[exp_name] = set(fovs[:n_train])

        def train_mask(df) -> np.ndarray:
            mask = np.zeros(len(df), dtype=bool)
            for exp_name, group in df.groupby("experiment", sort=False, observed=True):
                train_fovs = train_fovs_per_exp.get(exp_name, set())
                if train_fovs:
                    mask[group.index.to_numpy()] = group["fov_name"].isin(train_fovs).to_numpy()
            return mask

        def split(df, mask):
            return df.take(np.flatnonzero(mask)).reset_index(drop=True), df.take(np.flatnonzero(~mask)).reset_index(drop=True)

        def materialize_strings(df):
            for col in df.columns:
                s = df[col]
                if isinstance(s.dtype, pd.CategoricalDtype):
                    continue
                if pd.api.types.is_string_dtype(s) or str(s.dtype).startswith(("string", "Arrow")):
                    df[col] = s.astype("category")

        materialize_strings(full_index.tracks)
        materialize_strings(full_index.valid_anchors)
        train_tracks, val_tracks = split(full_index.tracks, train_mask(full_index.tracks))
        train_va, val_va = split(full_index.valid_anchors, train_mask(full_index.valid_anchors))
        kw = dict(positive_cell_source=self.positive_cell_source, positive_match_columns=self.positive_match_columns)
        self.train_dataset = self._dataset(full_index.clone_with_subset(
            train_tracks, max_border_shift=self.max_border_shift, precomputed_valid_anchors=train_va, **kw), fit=True)
        if not val_tracks.empty:
            self.val_dataset = self._dataset(full_index.clone_with_subset(val_tracks, precomputed_valid_anchors=val_va, **kw), fit=True)

    # ------------------------------------------------------------------ loaders (datamodule.py:611-715)
    def _ddp_topology(self) -> tuple[int, int]:
        trainer = getattr(self, "trainer", None)
        world_size, global_rank = getattr(trainer, "world_size", None), getattr(trainer, "global_rank", None)
        if world_size is None or global_rank is None:
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                return torch.distributed.get_world_size(), torch.distributed.get_rank()
            return 1, 0
        return world_size, global_rank

    def _sampler(self, ds, temporal_enrichment: bool) -> FlexibleBatchSampler:
        num_replicas, rank = self._ddp_topology()
        kw = dict(temporal_window_hours=self.temporal_window_hours, temporal_global_fraction=self.temporal_global_fraction) \
            if temporal_enrichment else {}
        return FlexibleBatchSampler(valid_anchors=ds.index.valid_anchors, batch_size=self.batch_size, batch_group_by=self.batch_group_by,
                                    leaky=self.leaky, group_weights=self.group_weights, stratify_by=self.stratify_by,
                                    temporal_enrichment=temporal_enrichment, num_replicas=num_replicas, rank=rank, seed=self.seed, **kw)

    def train_dataloader(self):
        return DataLoader(self.train_dataset, batch_sampler=self._sampler(self.train_dataset, self.temporal_enrichment),
                          num_workers=0, collate_fn=identity)

    def val_dataloader(self):
        if self.val_dataset is None:
            return None
        return DataLoader(self.val_dataset, batch_sampler=self._sampler(self.val_dataset, False), num_workers=0, collate_fn=identity)

    def predict_dataloader(self):
        return DataLoader(self.predict_dataset, batch_size=self.batch_size, num_workers=0, shuffle=False, drop_last=False,
                          collate_fn=identity)

    # ------------------------------------------------------------------ transforms (datamodule.py:721-824)
    def _train_final_crop(self):
        from ..transforms import BatchedCenterSpatialCropd

        return BatchedCenterSpatialCropd(keys=self._channel_names, roi_size=(self.z_window, *self.final_yx_patch_size))

    @staticmethod
    def _all_or_none(norm_meta, message: str):
        if isinstance(norm_meta, list):
            non_none = [m for m in norm_meta if m is not None]
            if len(non_none) == 0:
                return None
            if len(non_none) != len(norm_meta):
                raise ValueError(message)
        return norm_meta

    def _labelfree_mask(self, batch: dict, key: str) -> dict | None:
        if not isinstance(self.channels_per_sample, int):
            return None
        meta = batch.get(f"{key}_meta")
        if meta is None:
            return None
        flags = [parse_channel_name(m.get("marker", ""))["channel_type"] == "labelfree" for m in meta]
        return {"_is_labelfree": torch.tensor(flags, dtype=torch.bool, device=batch[key].device)}

    @torch.no_grad()
    def on_after_batch_transfer(self, batch, dataloader_idx: int):
        if isinstance(batch, Tensor):
            return batch
        if self.trainer is not None and getattr(self.trainer, "predicting", False):
            norm_meta = self._all_or_none(batch.get("anchor_norm_meta"), "Mixed None/non-None norm_meta in predict batch.")
            batch["anchor"] = transform_channel_wise(self._predict_transform, self._channel_names, batch["anchor"], norm_meta,
                                                      self._labelfree_mask(batch, "anchor"))
            batch.pop("anchor_norm_meta", None)
            batch.pop("anchor_meta", None)
            return batch
        for key in ["anchor", "positive", "negative"]:
            if key in batch:
                norm_meta_key = f"{key}_norm_meta"
                norm_meta = self._all_or_none(batch.get(norm_meta_key), f"Mixed None/non-None norm_meta in batch for '{key}'. "
                                              "All FOVs must have normalization metadata or none of them.")
                batch[key] = transform_channel_wise(self._augmentation_transform, self._channel_names, batch[key], norm_meta,
                                                     self._labelfree_mask(batch, key))
                if norm_meta_key in batch:
                    del batch[norm_meta_key]
        for key in ["anchor", "positive"]:
            if key in batch:
                batch[key] = self.channel_dropout(batch[key])
        return batch
