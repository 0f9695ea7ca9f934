"""Host restatement of ``viscy preprocess`` (viscy_utils/mp_utils.py get_val_stats, viscy_utils/meta_utils.py
generate_normalization_metadata / generate_fg_masks) over numpy arrays: numpy's own nanpercentile / nanmin / nanmax / nanmean /
nanstd, ``scipy.ndimage.median_filter`` and the rule of ``skimage.filters.threshold_otsu`` (scikit-image is not installed: the rule
is ``viscy_amd.preprocess.otsu_from_histogram`` on ``np.bincount`` / ``np.histogram``).  Nothing here touches a device or a store:
positions are ``{"A/1/0": array(T, C, Z, Y, X)}``."""

import numpy as np

PERCENTILES = [1, 5, 25, 50, 75, 95, 99]


def get_val_stats(sample_values):
    pv = dict(zip(PERCENTILES, (float(v) for v in np.nanpercentile(sample_values, PERCENTILES))))
    return {
        "min": float(np.nanmin(sample_values)),
        "max": float(np.nanmax(sample_values)),
        "mean": float(np.nanmean(sample_values)),
        "std": float(np.nanstd(sample_values)),
        "median": pv[50],
        "iqr": pv[75] - pv[25],
        "p5": pv[5],
        "p95": pv[95],
        "p95_p5": pv[95] - pv[5],
        "p1": pv[1],
        "p99": pv[99],
        "p99_p1": pv[99] - pv[1],
    }


def golden_cases():
    """name -> array: the seeded inputs of tests/golden/preprocess_stats.json (tools/gen_golden_preprocess.py records the
    reference's get_val_stats on exactly these)"""
    rng = np.random.default_rng(20240521)
    cases = {}
    cases["uint16"] = rng.integers(0, 65536, size=(3, 5, 19, 13), dtype=np.uint16)
    cases["uint16_narrow"] = rng.integers(100, 140, size=(2, 3, 11, 7), dtype=np.uint16)
    cases["float32"] = (rng.standard_normal((3, 5, 19, 13)) * 37.5 + 410.0).astype(np.float32)
    nan = (rng.standard_normal((2, 4, 23, 9)) * 3.0).astype(np.float32)
    nan.reshape(-1)[rng.permutation(nan.size)[:97]] = np.nan
    nan.reshape(-1)[[0, -1]] = np.nan
    cases["float32_nan"] = nan
    cases["uint16_one"] = np.array([[[[40000]]]], dtype=np.uint16)
    cases["float32_one"] = np.array([[[[-3.25]]]], dtype=np.float32)
    return cases


def grid_sample(arr, g, c):
    """meta_utils.py _grid_sample: (T, Z, ceil(Y / g), ceil(X / g))"""
    return arr[:, c, :, ::g, ::g]


def otsu_histogram(flat):
    """(counts, centres) as skimage's histogram makes them: one bin per integer from min to max for integer data,
    ``np.histogram(flat, 256)`` with the centres of its edges for float data"""
    if np.issubdtype(flat.dtype, np.integer):
        lo, hi = int(flat.min()), int(flat.max())
        return np.bincount(flat.astype(np.int64) - lo, minlength=hi - lo + 1), np.arange(lo, hi + 1)
    counts, e = np.histogram(flat, 256)
    return counts, (e[:-1] + e[1:]) / 2


def otsu_threshold(otsu_samples):
    """meta_utils.py:116-125 on the (T, Z, y, x) Otsu sample"""
    from scipy.ndimage import median_filter

    from viscy_amd.preprocess import otsu_from_histogram

    flat = median_filter(otsu_samples, size=(1, 1, 3, 3)).ravel()
    if flat.min() == flat.max():
        return float(flat.min())
    return otsu_from_histogram(*otsu_histogram(flat))


def normalization_metadata(positions, channel_names, channel_ids=-1, grid_spacing=32, compute_otsu=False, otsu_grid_spacing=8):
    """-> (plate_meta, {position: meta}): what ``.zattrs["normalization"]`` of the plate and of every position holds afterwards"""
    if channel_ids == -1:
        channel_ids = range(len(channel_names))
    elif isinstance(channel_ids, int):
        channel_ids = [channel_ids]
    T = next(iter(positions.values())).shape[0]
    plate_meta, pos_meta = {}, {name: {} for name in positions}
    for c in channel_ids:
        samples_all, per_pos = [], {}
        for name, arr in positions.items():
            samples = grid_sample(arr, grid_spacing, c)
            samples_all.append(samples)
            fov = get_val_stats(samples)
            if compute_otsu:
                fov["otsu_threshold"] = otsu_threshold(grid_sample(arr, otsu_grid_spacing, c))
            per_pos[name] = {"fov_statistics": fov, "timepoint_statistics": {str(t): get_val_stats(samples[t]) for t in range(T)}}
        dataset = {"dataset_statistics": get_val_stats(np.stack(samples_all))}
        per_t = {str(t): get_val_stats(np.stack([s[t] for s in samples_all])) for t in range(T)}
        plate_meta[channel_names[c]] = dataset | {"timepoint_statistics": per_t}
        for name in positions:
            pos_meta[name][channel_names[c]] = dataset | per_pos[name]
    return plate_meta, pos_meta


def fg_masks(positions, channel_names, target_names, pos_meta):
    """-> {position: uint8 (T, C, Z, Y, X)}: 1 for the channels not named, median >= threshold for the named ones"""
    from scipy.ndimage import median_filter

    out = {}
    for name, arr in positions.items():
        mask = np.zeros(arr.shape, dtype=np.uint8)
        targets = [channel_names.index(n) for n in target_names]
        for c in sorted(set(range(arr.shape[1])) - set(targets)):
            mask[:, c] = 1
        for n, c in zip(target_names, targets):
            thr = pos_meta[name][n]["fov_statistics"]["otsu_threshold"]
            for t in range(arr.shape[0]):
                smoothed = median_filter(arr[t, c].astype(np.float32), size=(1, 3, 3))
                mask[t, c] = (smoothed >= thr).astype(np.uint8)
        out[name] = mask
    return out


def bimodal_plate(dtype, seed=11, n_pos=2, shape=(2, 2, 3, 40, 72)):
    """positions of the end-to-end tests: a dim background with bright square blobs, a different layout per position, time point
    and channel; uint16 counts or float32 intensities"""
    rng = np.random.default_rng(seed)
    T, C, Z, Y, X = shape
    positions = {}
    for i in range(n_pos):
        img = rng.normal(300.0, 25.0, size=shape)
        for t in range(T):
            for c in range(C):
                for _ in range(5):
                    y, x = int(rng.integers(0, Y - 10)), int(rng.integers(0, X - 14))
                    img[t, c, :, y:y + 10, x:x + 14] += rng.normal(2200.0 + 400.0 * c, 60.0, size=(Z, 10, 14))
        img = np.clip(img, 0, 65535)
        positions[f"A/{i + 1}/0"] = np.round(img).astype(np.uint16) if np.dtype(dtype) == np.uint16 else (img / 7.0).astype(np.float32)
    return positions
