"""``viscy preprocess`` on the MI355X: the normalisation statistics, Otsu thresholds and foreground masks that ``NormalizeSampled``,
``TripletDataModule`` and ``SpotlightLoss(fg_mask)`` read from a store (``viscy_utils.meta_utils.generate_normalization_metadata`` /
``generate_fg_masks``, ``viscy_utils.mp_utils.get_val_stats``; ``VisCyTrainer.preprocess`` is ``viscy_amd.trainer.Trainer.preprocess``).

Store decode stays on the host (``viscy_amd.data.ome_zarr``); every frame is decoded once and uploaded once in its storage dtype.  On
the device (csrc/preprocess.hip, csrc/boc_transforms.hip):

* ``vsx_grid_sample``  the ``[:, ::g, ::g]`` sample of a frame, fp32
* ``vsx_median3x3``    scipy's 3 x 3 ``median_filter`` of the Otsu sample, and of every full-resolution target plane with the
                       ``>= threshold`` comparison in its epilogue (the mask leaves the kernel as uint8)
* ``vsx_nan_moments``  count / min / max / sum, then the centred sums: fixed-order float64, exact int64 for integer stores
* ``vsx_row_select``   the two exact neighbouring order statistics of every percentile (no sort)
* ``vsx_hist_int`` / ``vsx_hist_edges``  the histogram Otsu scans

and on the host, in float64: numpy's percentile interpolation (``percentiles_from_order_stats``) and the Otsu scan
(``otsu_from_histogram``), both pure functions.  Stated differences from the reference are listed in INTEGRATION.md ("preprocess").
There is no CPU fallback: without a HIP device ``get_val_stats`` and the two ``generate_*`` functions raise.
"""

from __future__ import annotations

import json
import math
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from torch import Tensor

from ._lib import check, lib, ptr, stream
from .data.ome_zarr import open_ome_zarr
from .ops import frame_dtype_code

PERCENTILES = (1, 5, 25, 50, 75, 95, 99)
STAT_KEYS = ("min", "max", "mean", "std", "median", "iqr", "p5", "p95", "p95_p5", "p1", "p99", "p99_p1")
MAX_SAMPLE = 2 ** 31 - 1
MAX_WORKERS = 16
_INTEGRAL_NP = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int16))
_INTEGRAL_T = (torch.uint8, torch.uint16, torch.int16)


# ------------------------------------------------------------------------------------------------ pure host functions
def percentile_ranks(n: int, percentiles=PERCENTILES) -> tuple[list[int], list[int], np.ndarray]:
    """numpy's method="linear" on ``n`` sorted values (``np.percentile`` -> ``_quantile``): for every percentile the zero-based ranks
    of the two neighbours and the weight ``gamma`` between them, float64.  ``virtual = (n - 1) * (q / 100)``; a virtual index at or
    past the last element takes the last element twice, and numpy's gamma is then ``virtual + 1`` (both neighbours are equal)."""
    q = np.true_divide(np.asarray(percentiles), 100)
    virtual = (n - 1) * q
    prev = np.floor(virtual)
    nxt = prev + 1
    above = virtual >= n - 1
    prev[above], nxt[above] = -1, -1
    below = virtual < 0
    prev[below], nxt[below] = 0, 0
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asanyarray(virtual - prev, dtype=virtual.dtype)
    return [int(i) % n for i in prev], [int(i) % n for i in nxt], gamma


def percentiles_from_order_stats(lower, upper, gamma) -> np.ndarray:
    """numpy's ``_lerp`` on the exact neighbouring order statistics: ``lower[i] + (upper[i] - lower[i]) * gamma[i]``, and
    ``upper[i] - (upper[i] - lower[i]) * (1 - gamma[i])`` where ``gamma[i] >= 0.5``.  ``lower`` / ``upper`` keep the dtype of the
    data: the difference is formed in it (float32 for float32 data, as numpy does), everything after in float64.  Returns float64."""
    a, b = np.asarray(lower), np.asarray(upper)
    t = np.asarray(gamma, dtype=np.float64)
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * t), dtype=np.float64)
    np.subtract(b, diff * (1 - t), out=out, where=t >= 0.5, casting="unsafe", dtype=np.float64)
    return out


def otsu_from_histogram(counts, centers) -> float:
    """The rule of ``skimage.filters.threshold_otsu`` on a histogram, in float64: the centre of the first bin that maximises the
    inter-class variance.  One bin (a constant image) gives its centre."""
    c, b = np.asarray(counts, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    if c.shape != b.shape or c.ndim != 1 or c.size == 0:
        raise ValueError(f"otsu_from_histogram: counts {c.shape} and centers {b.shape} must be equal, non-empty 1-D")
    if c.size == 1:
        return float(b[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = np.cumsum(c)
        w2 = np.cumsum(c[::-1])[::-1]
        m1 = np.cumsum(c * b) / w1
        m2 = (np.cumsum((c * b)[::-1]) / w2[::-1])[::-1]
        v = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return float(b[int(np.argmax(v))])


def _stats_dict(vmin: float, vmax: float, mean: float, std: float, pct) -> dict:
    p = {k: float(v) for k, v in zip(PERCENTILES, pct)}
    return {"min": float(vmin), "max": float(vmax), "mean": float(mean), "std": float(std), "median": p[50], "iqr": p[75] - p[25],
            "p5": p[5], "p95": p[95], "p95_p5": p[95] - p[5], "p1": p[1], "p99": p[99], "p99_p1": p[99] - p[1]}


def write_meta_field(position, metadata: dict, field_name: str, subfield_name: str) -> None:
    """meta_utils.py write_meta_field on a ``viscy_amd.data.ome_zarr`` node (plate or position): a new field, a new subfield of an
    existing field, or an existing subfield updated key by key; then the node's ``.zattrs`` is rewritten."""
    if getattr(position, "v3", False):
        raise NotImplementedError("zarr v3 stores are read-only here")
    attrs = position.zattrs
    if field_name in attrs:
        if subfield_name in attrs[field_name]:
            attrs[field_name] = {**attrs[field_name], subfield_name: {**attrs[field_name][subfield_name], **metadata}}
        else:
            attrs[field_name] = {**attrs[field_name], subfield_name: metadata}
    else:
        attrs[field_name] = {subfield_name: metadata}
    (position.fs_path / ".zattrs").write_text(json.dumps(attrs))


# ------------------------------------------------------------------------------------------------ device wrappers
def _device(who: str) -> torch.device:
    from .evalkit import device_of

    return device_of(who=who)


def _planes(src: Tensor, who: str) -> tuple[int, int, int, int, int, int]:
    """(dtype code, z stride, y stride, Z, H, W) of a [Z, H, W] device view the kernels read as it is"""
    if not (torch.is_tensor(src) and src.is_cuda and src.ndim == 3 and src.numel() > 0):
        raise RuntimeError(f"{who} needs a non-empty [Z, H, W] tensor on the HIP device (no CPU fallback)")
    code = frame_dtype_code(src.dtype, who)
    Z, H, W = src.shape
    sz, sy, sx = src.stride()
    if (W > 1 and sx != 1) or sz < 0 or (H > 1 and sy < W) or (H == 1 and sy < 0):
        raise ValueError(f"{who}: strides {src.stride()} of a {tuple(src.shape)} view: x must be contiguous, rows must not overlap")
    return code, sz, max(sy, W), Z, H, W


def _out(out: Tensor | None, shape, dtype, dev, who: str) -> Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (out.is_cuda and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous {dtype} device tensor of shape {tuple(shape)}")
    return out


def grid_sample(src: Tensor, g: int, out: Tensor | None = None) -> Tensor:
    """``src[:, ::g, ::g]`` of a [Z, H, W] device view as float32 (``vsx_grid_sample``)"""
    code, sz, sy, Z, H, W = _planes(src, "preprocess.grid_sample")
    g = int(g)
    if g < 1:
        raise ValueError(f"grid spacing {g} < 1")
    out = _out(out, (Z, -(-H // g), -(-W // g)), torch.float32, src.device, "preprocess.grid_sample")
    check(lib().vsx_grid_sample(src.data_ptr(), code, sz, sy, Z, H, W, g, ptr(out), stream()), "grid_sample")
    return out


def median3x3(src: Tensor, out: Tensor | None = None) -> Tensor:
    """``scipy.ndimage.median_filter(src, size=(1, 3, 3))`` of a float32 [Z, H, W] device view (NaN-free), float32"""
    code, sz, sy, Z, H, W = _planes(src, "preprocess.median3x3")
    if src.dtype != torch.float32:
        raise NotImplementedError("preprocess.median3x3 smooths float32 samples; typed frames go through median3x3_mask")
    out = _out(out, (Z, H, W), torch.float32, src.device, "preprocess.median3x3")
    check(lib().vsx_median3x3(src.data_ptr(), code, sz, sy, Z, H, W, ptr(out), None, 0.0, stream()), "median3x3")
    return out


def median3x3_mask(src: Tensor, threshold: float, out: Tensor | None = None) -> Tensor:
    """``(median_filter(src.astype(float32), size=(1, 3, 3)) >= threshold).astype(uint8)`` of a typed [Z, H, W] device view; the
    threshold is rounded to float32, which is what numpy's comparison of a float32 array with a Python float does"""
    code, sz, sy, Z, H, W = _planes(src, "preprocess.median3x3_mask")
    out = _out(out, (Z, H, W), torch.uint8, src.device, "preprocess.median3x3_mask")
    thr = float(np.float32(threshold))
    check(lib().vsx_median3x3(src.data_ptr(), code, sz, sy, Z, H, W, None, ptr(out), thr, stream()), "median3x3_mask")
    return out


def _row(x: Tensor, who: str) -> Tensor:
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and 1 <= x.numel() <= MAX_SAMPLE):
        raise RuntimeError(f"{who} needs a contiguous float32 tensor of 1 .. 2^31 - 1 values on the HIP device (no CPU fallback)")
    return x.reshape(-1)


def nan_moments(x: Tensor, *, integral: bool = False, mean: float | None = None) -> tuple[Tensor, Tensor | None]:
    """``vsx_nan_moments`` on a contiguous float32 device tensor.  ``mean`` None: pass 1, -> (float64 [4] {count of non-NaN values,
    min, max, sum}, int64 [2] {sum x, sum x^2} where ``integral`` else None).  ``mean`` given: pass 2, -> (float64 [4]
    {sum (x - mean)^2, sum (x - mean), 0, 0}, None).  The results stay on the device."""
    x = _row(x, "preprocess.nan_moments")
    n = x.numel()
    nbytes = lib().vsx_nan_moments_ws_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
    out = torch.empty(4, dtype=torch.float64, device=x.device)
    isums = torch.empty(2, dtype=torch.int64, device=x.device) if integral and mean is None else None
    check(lib().vsx_nan_moments(ptr(x), n, 1 if mean is None else 2, int(isums is not None), 0.0 if mean is None else float(mean),
                                ptr(out), ptr(isums), ptr(ws), nbytes, stream()), "nan_moments")
    return out, isums


def hist_int(x: Tensor, lo: int, nbins: int) -> Tensor:
    """counts [nbins] (int64 view of the kernel's uint64) of the integer-valued float32 values of ``x`` in [lo, lo + nbins)"""
    x = _row(x, "preprocess.hist_int")
    counts = torch.empty(int(nbins), dtype=torch.int64, device=x.device)
    check(lib().vsx_hist_int(ptr(x), x.numel(), int(lo), int(nbins), ptr(counts), stream()), "hist_int")
    return counts


def hist_edges(x: Tensor, edges) -> Tensor:
    """``np.histogram(x, bins=edges)[0]`` for ascending edges (any float dtype; compared in float64): int64 counts on the device"""
    x = _row(x, "preprocess.hist_edges")
    e = torch.as_tensor(np.ascontiguousarray(np.asarray(edges, dtype=np.float64))).to(x.device)
    counts = torch.empty(e.numel() - 1, dtype=torch.int64, device=x.device)
    check(lib().vsx_hist_edges(ptr(x), x.numel(), ptr(e), e.numel() - 1, ptr(counts), stream()), "hist_edges")
    return counts


def _order_stats(x: Tensor, ranks: list[int]) -> dict[int, float]:
    """{rank: sorted(x)[rank]} of a NaN-free float32 row: ``vsx_row_select`` takes four ranks a call, duplicates removed first"""
    from .transforms import row_select

    uniq = sorted(set(ranks))
    row = x.reshape(1, -1)
    parts = [row_select(row, uniq[i:i + 4]) for i in range(0, len(uniq), 4)]
    vals = torch.cat(parts, dim=1)[0].cpu().numpy()
    return dict(zip(uniq, vals))


# ------------------------------------------------------------------------------------------------ get_val_stats
def _val_stats(x: Tensor, integral: bool, np_dtype) -> dict:
    """x: contiguous float32 device tensor; ``integral``: it holds integers of a uint8 / uint16 / int16 store; ``np_dtype``: the
    dtype the order statistics are handed to numpy's interpolation in"""
    x = _row(x, "preprocess.get_val_stats")
    out, isums = nan_moments(x, integral=integral)
    cnt_f, vmin, vmax, total = out.cpu().tolist()
    cnt = int(cnt_f)
    if cnt == 0:
        return dict.fromkeys(STAT_KEYS, float("nan"))
    if cnt < x.numel():
        x = x[~torch.isnan(x)].contiguous()
    lo, hi, gamma = percentile_ranks(cnt)
    m2 = None
    if not integral:
        mean = total / cnt
        m2 = nan_moments(x, mean=mean)[0]
    stats = _order_stats(x, lo + hi)
    pct = percentiles_from_order_stats(np.array([stats[r] for r in lo]).astype(np_dtype), np.array([stats[r] for r in hi]).astype(np_dtype), gamma)
    if integral:
        s1, s2 = (int(v) for v in isums.cpu().tolist())
        mean = s1 / cnt                                        # integers: one correctly rounded division
        std = math.sqrt((cnt * s2 - s1 * s1) / (cnt * cnt))    # the exact variance as a ratio of integers, rounded once
    else:
        d2, d1, _, _ = m2.cpu().tolist()
        std = math.sqrt(max((d2 - d1 * d1 / cnt) / cnt, 0.0))  # the two-pass sum with its first-order correction
    return _stats_dict(vmin, vmax, mean, std, pct)


def get_val_stats(sample_values) -> dict:
    """``viscy_utils.mp_utils.get_val_stats``: the same twelve keys in the same order, Python floats.  A numpy array (uint8 / uint16 /
    int16 / float32) is uploaded; a device tensor of one of those dtypes is used where it is.  min, max and the percentile keys are
    numpy's values exactly; mean and std are the float64 values (exact integer sums for integer data): for float32 data numpy forms
    them in float32."""
    dev = _device("preprocess.get_val_stats")
    if torch.is_tensor(sample_values):
        t = sample_values.detach()
        if t.dtype not in _INTEGRAL_T and t.dtype != torch.float32:
            raise NotImplementedError(f"get_val_stats: {t.dtype} samples are not built (float32, uint16, int16, uint8 are)")
        integral = t.dtype in _INTEGRAL_T
        np_dtype = np.dtype(str(t.dtype).replace("torch.", ""))
        x = t.to(dev).contiguous()
        if integral and x.numel():  # the exact conversion of the sampling kernel at spacing 1
            x = grid_sample(x.view(1, 1, -1), 1).view(-1)
    else:
        a = np.asarray(sample_values)
        if a.dtype not in _INTEGRAL_NP and a.dtype != np.float32:
            raise NotImplementedError(f"get_val_stats: {a.dtype} samples are not built (float32, uint16, int16, uint8 are)")
        integral, np_dtype = a.dtype in _INTEGRAL_NP, a.dtype
        x = torch.from_numpy(np.ascontiguousarray(a).astype(np.float32, copy=False)).to(dev)
    if x.numel() == 0:
        raise ValueError("get_val_stats: empty sample")
    return _val_stats(x, integral, np_dtype)


# ------------------------------------------------------------------------------------------------ Otsu
def float_hist_edges(vmin: float, vmax: float, nbins: int = 256) -> np.ndarray:
    """the edges ``np.histogram(x, nbins)`` produces for float32 data with this min and max (float32, as numpy makes them)"""
    return np.histogram_bin_edges(np.array([vmin, vmax], dtype=np.float32), bins=nbins)


def otsu_threshold(smoothed: Tensor, integral: bool) -> float:
    """meta_utils.py:118-125 on the smoothed sample (float32, device, NaN-free): the constant for a constant sample, else Otsu's
    threshold of the device's histogram: one bin per integer for integer stores, ``np.histogram(x, 256)`` for float stores"""
    x = _row(smoothed, "preprocess.otsu_threshold")
    _, vmin, vmax, _ = nan_moments(x)[0].cpu().tolist()
    if vmin == vmax:
        return float(vmin)
    if integral:
        lo, hi = int(vmin), int(vmax)
        counts = hist_int(x, lo, hi - lo + 1).cpu().numpy()
        return otsu_from_histogram(counts, np.arange(lo, hi + 1))
    edges = float_hist_edges(vmin, vmax)
    counts = hist_edges(x, edges).cpu().numpy()
    return otsu_from_histogram(counts, (edges[:-1] + edges[1:]) / 2)


# ------------------------------------------------------------------------------------------------ the two generate_* functions
def _open_v2(zarr_dir):
    plate = open_ome_zarr(zarr_dir, mode="r+")
    if getattr(plate, "v3", False):
        raise NotImplementedError("zarr v3 stores are read-only here")
    return plate


def _frame_dtype(img) -> tuple[torch.dtype, bool]:
    dt = np.dtype(img.dtype)
    if dt not in _INTEGRAL_NP and dt != np.float32:
        raise NotImplementedError(f"preprocess: images stored as {dt} are not built (float32, uint16, int16, uint8 are)")
    return getattr(torch, dt.name), dt in _INTEGRAL_NP


class _Clock:
    """wall-clock seconds per stage, taken only where the caller asks for them (tools/perf_preprocess.py): the device stage is closed by a
    synchronise, so a run that is timed is a run that waits"""

    def __init__(self, timings: dict | None):
        self.t = timings

    def add(self, key: str, t0: float, sync: bool = False) -> float:
        if self.t is not None:
            if sync:
                torch.cuda.synchronize()
            self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t0
        return time.perf_counter()


def generate_normalization_metadata(zarr_dir, num_workers: int = 4, channel_ids=-1, grid_spacing: int = 32, compute_otsu: bool = False,
                                    otsu_grid_spacing: int = 8, *, timings: dict | None = None) -> None:
    """meta_utils.py generate_normalization_metadata: the plate's ``.zattrs["normalization"][channel]`` gets ``dataset_statistics`` +
    ``timepoint_statistics``, every position's gets ``dataset_statistics`` + ``fov_statistics`` (with ``otsu_threshold`` when
    ``compute_otsu``) + ``timepoint_statistics``.  A channel's sample lives on the device as [T, P, Z, h, w]: a time point's slab and the
    whole are contiguous rows.  ``num_workers`` (at most 16) sizes the host decode pool."""
    plate = _open_v2(zarr_dir)
    dev = _device("preprocess.generate_normalization_metadata")
    clock = _Clock(timings)
    position_map = list(plate.positions())
    if not position_map:
        raise ValueError(f"{zarr_dir}: the plate has no positions")
    names = plate.channel_names
    if channel_ids == -1:
        channel_ids = range(len(names))
    elif isinstance(channel_ids, int):
        channel_ids = [channel_ids]
    images = [pos["0"] for _, pos in position_map]
    shapes = {tuple(img.shape[0:1] + img.shape[2:]) for img in images}
    if len(shapes) != 1:
        raise ValueError("all input arrays must have the same shape")  # np.stack's words: the positions' (T, Z, Y, X) differ
    tdtype, integral = _frame_dtype(images[0])
    if any(np.dtype(img.dtype) != np.dtype(images[0].dtype) for img in images):
        raise ValueError("preprocess: the positions of a plate must share one storage dtype")
    T, _, Z, H, W = images[0].shape
    P, g, go = len(images), int(grid_spacing), int(otsu_grid_spacing)
    if g < 1 or go < 1:
        raise ValueError(f"grid spacings must be >= 1, got {g} and {go}")
    h, w, ho, wo = -(-H // g), -(-W // g), -(-H // go), -(-W // go)
    total = T * P * Z * h * w
    # resident at once: the [T, P, Z, h, w] sample, one copy of it (a position's rows, or the NaN-free compaction) and the row-select
    # scratch; with Otsu the position's denser sample twice; one frame in its storage dtype
    need = 4 * total * 3 + (8 * T * Z * ho * wo if compute_otsu else 0) + Z * H * W * np.dtype(images[0].dtype).itemsize
    if total > MAX_SAMPLE or (compute_otsu and T * Z * ho * wo > MAX_SAMPLE):
        raise ValueError(f"preprocess: a dataset sample of {total} values exceeds 2^31 - 1: raise grid_spacing")
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise MemoryError(f"preprocess: the dataset sample needs about {need} bytes of device memory, {free} are free: raise grid_spacing")
    np_dtype = np.dtype(images[0].dtype)
    print(f"Detected {T} timepoints in dataset")
    with ThreadPoolExecutor(max(1, min(int(num_workers), MAX_WORKERS))) as pool:
        for i, c in enumerate(channel_ids):
            print(f"Sampling channel index {c} ({i + 1}/{len(channel_ids)})")
            channel_name = names[c]
            sample = torch.empty((T, P, Z, h, w), dtype=torch.float32, device=dev)
            position_and_statistics = []
            for p, (_, pos) in enumerate(position_map):
                t0 = time.perf_counter()
                frames = pool.map(lambda t, p=p, c=c: position_map[p][1]["0"].read_zrange(t, c, 0, Z), range(T))
                otsu = torch.empty((T, Z, ho, wo), dtype=torch.float32, device=dev) if compute_otsu else None
                for t, frame in enumerate(frames):
                    t0 = clock.add("decode", t0)
                    dframe = torch.from_numpy(frame).to(dev)
                    t0 = clock.add("upload", t0, sync=True)
                    grid_sample(dframe, g, out=sample[t, p])
                    if compute_otsu:
                        grid_sample(dframe, go, out=otsu[t])
                    t0 = clock.add("device", t0, sync=True)
                fov = sample[:, p].contiguous()
                fov_stats = _val_stats(fov, integral, np_dtype)
                if compute_otsu:
                    fov_stats["otsu_threshold"] = otsu_threshold(median3x3(otsu.view(T * Z, ho, wo)), integral)
                fov_statistics = {"fov_statistics": fov_stats,
                                  "timepoint_statistics": {str(t): _val_stats(sample[t, p], integral, np_dtype) for t in range(T)}}
                position_and_statistics.append((pos, fov_statistics))
                clock.add("device", t0, sync=True)
            t0 = time.perf_counter()
            dataset_statistics = {"dataset_statistics": _val_stats(sample, integral, np_dtype)}
            print(f"Computing per-timepoint statistics for channel {channel_name}")
            dataset_timepoint_statistics = {str(t): _val_stats(sample[t], integral, np_dtype) for t in range(T)}
            t0 = clock.add("device", t0, sync=True)
            write_meta_field(plate, dataset_statistics | {"timepoint_statistics": dataset_timepoint_statistics}, "normalization", channel_name)
            for pos, position_statistics in position_and_statistics:
                write_meta_field(pos, dataset_statistics | position_statistics, "normalization", channel_name)
            clock.add("write", t0)


def generate_fg_masks(zarr_dir, channel_names, fg_mask_key: str = "fg_mask", *, timings: dict | None = None) -> None:
    """meta_utils.py generate_fg_masks: a uint8 [T, C, Z, Y, X] array ``fg_mask_key`` next to every position's image: 1 for the
    channels not named, ``median_filter(frame, (1, 3, 3)) >= otsu_threshold`` for the named ones, time point by time point.  Unlike
    the reference, every refusal (``FileExistsError``: the key exists; ``KeyError``: a channel without ``otsu_threshold``) comes before
    the first array is created."""
    plate = _open_v2(zarr_dir)
    all_channel_names = plate.channel_names
    channel_names = list(channel_names)
    channel_indices = [all_channel_names.index(name) for name in channel_names]
    position_map = list(plate.positions())
    thresholds = {}
    for pos_name, pos in position_map:
        if fg_mask_key in pos:
            raise FileExistsError(f"Mask array '{fg_mask_key}' already exists at {pos_name}. Delete it first to regenerate.")
    for pos_name, pos in position_map:
        for ch_name in channel_names:
            thresholds[pos_name, ch_name] = pos.zattrs["normalization"][ch_name]["fov_statistics"]["otsu_threshold"]
        _frame_dtype(pos["0"])
    dev = _device("preprocess.generate_fg_masks")
    clock = _Clock(timings)
    for pos_name, pos in position_map:
        img_arr = pos["0"]
        t_total, c_total = img_arr.shape[0], img_arr.shape[1]
        zyx_shape = tuple(img_arr.shape[2:])
        src_chunks = img_arr.chunks
        mask_chunks = (1, 1, min(src_chunks[2], zyx_shape[0]), min(src_chunks[3], 512), min(src_chunks[4], 512))
        t0 = time.perf_counter()
        mask_arr = pos.create_zeros(fg_mask_key, shape=(t_total, c_total, *zyx_shape), dtype=np.uint8, chunks=mask_chunks)
        ones = np.ones(zyx_shape, dtype=np.uint8)
        for c in sorted(set(range(c_total)) - set(channel_indices)):
            for t in range(t_total):
                mask_arr.write_zrange(t, c, 0, ones)
        t0 = clock.add("write", t0)
        for ch_name, ch_idx in zip(channel_names, channel_indices):
            thr = thresholds[pos_name, ch_name]
            for t in range(t_total):
                frame = img_arr.read_zrange(t, ch_idx, 0, zyx_shape[0])
                t0 = clock.add("decode", t0)
                dframe = torch.from_numpy(frame).to(dev)
                t0 = clock.add("upload", t0, sync=True)
                mask = median3x3_mask(dframe, thr)
                t0 = clock.add("device", t0, sync=True)
                host = mask.cpu().numpy()
                t0 = clock.add("download", t0)
                mask_arr.write_zrange(t, ch_idx, 0, host)
                t0 = clock.add("write", t0)
