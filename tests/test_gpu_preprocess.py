"""GPU: the kernels of csrc/preprocess.hip behind ``viscy_amd.preprocess``, and ``viscy preprocess`` end to end.

Every source is a strided view into a larger [T, C, Z, H, W] block (rows wider than the view, an odd element offset); every output
sits between guard rows and starts poisoned (NaN bits / 0xFF); every kernel runs twice and must give the same bits.  Shapes come
from the kernels' constants (``VSX_MEDIAN_COLS`` / ``VSX_MEDIAN_ROWS``: a wave's strip; ``VSX_MOMENTS_CHUNK``: a workgroup's partial;
``VSX_HIST_LDS_BINS``: private against global counters).  Tolerances, where a result is not exact, are derived where they are used."""

import math
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.ndimage import median_filter

from tests import ref_preprocess as RP

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
DTYPES = ["float32", "uint16", "int16", "uint8"]
GUARD_BITS = 0x7FC0DEAD


@pytest.fixture(scope="module")
def PP():
    from viscy_amd import preprocess

    return preprocess


@pytest.fixture(scope="module")
def K():
    from viscy_amd import _lib

    return _lib


def make_block(rng, dtype, shape, bits=False):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        if bits:  # random bit patterns: NaNs with payloads, infinities and denormals among them (copies only)
            return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)
        return (rng.standard_normal(shape) * 100.0).astype(np.float32)
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max + 1, size=shape).astype(dtype)
    a.reshape(-1)[:2] = (info.min, info.max)
    return a


def strided_view(rng, dtype, Z, H, W, bits=False):
    """(numpy view [Z, H, W], device view of the same elements) cut out of a [2, 3, Z, H + 3, W + 5] block at t = 1, c = 2, y0 = 2,
    x0 = 3: the row stride exceeds W and the first element sits at an odd offset"""
    block = make_block(rng, dtype, (2, 3, Z, H + 3, W + 5), bits)
    dev = torch.from_numpy(block).to(DEV)
    return block[1, 2, :, 2:2 + H, 3:3 + W], dev[1, 2, :, 2:2 + H, 3:3 + W]


def guarded(shape, dtype):
    """(whole buffer, the output view inside it, guard length): float32 outputs are poisoned with a NaN pattern, uint8 with 0xFF"""
    total = int(np.prod(shape))
    guard = 64
    if dtype == torch.float32:
        buf = torch.full((guard + total + guard,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    else:
        buf = torch.full((guard + total + guard,), 0xFF, dtype=torch.uint8, device=DEV)
    return buf, buf[guard:guard + total].view(shape), guard


def raw(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.uint8).cpu().numpy()


def run_guarded(fn, shape, dtype):
    """calls ``fn(out)`` twice into fresh guarded buffers; -> the output's raw bits (checked equal between the runs, guards intact)"""
    got = []
    for _ in range(2):
        buf, out, guard = guarded(shape, dtype)
        res = fn(out)
        assert res.data_ptr() == out.data_ptr()
        bits = raw(buf)
        poison = GUARD_BITS if dtype == torch.float32 else 0xFF
        assert (bits[:guard] == poison).all() and (bits[-guard:] == poison).all(), "guard rows were written"
        got.append(bits[guard:-guard].reshape(shape))
    assert np.array_equal(got[0], got[1]), "two runs differ"
    return got[0]


# ------------------------------------------------------------------------------------------------ vsx_grid_sample
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [32, 1, 100])
def test_grid_sample_equals_numpy_slicing(PP, dtype, g):
    Z, H, W = 3, 65, 33   # g = 32: rows 0, 32, 64 and columns 0, 32; g = 100 > H: one sample per plane
    rng = np.random.default_rng(100 + g)
    host, dev = strided_view(rng, dtype, Z, H, W, bits=True)
    want = host[:, ::g, ::g].astype(np.float32)
    assert want.shape == (Z, -(-H // g), -(-W // g))
    got = run_guarded(lambda out: PP.grid_sample(dev, g, out=out), want.shape, torch.float32)
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.int32))


def test_grid_sample_refusals(PP):
    x = torch.zeros((2, 8, 8), device=DEV)
    with pytest.raises(ValueError):
        PP.grid_sample(x, 0)
    with pytest.raises(ValueError):
        PP.grid_sample(x.transpose(1, 2), 2)               # x is not contiguous
    with pytest.raises(NotImplementedError):
        PP.grid_sample(x.to(torch.float64), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.grid_sample(x.cpu(), 2)


# ------------------------------------------------------------------------------------------------ vsx_median3x3
def median_shapes(K):
    c, r = K.MEDIAN_COLS, K.MEDIAN_ROWS
    # one past a wave's strip in both directions (four strips a plane), and the strip itself with one row / column less
    return [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (r + 1, c + 1), (r - 1, c - 1), (2 * r + 1, 2 * c + 1)]


def test_median_float_equals_scipy(PP, K):
    rng = np.random.default_rng(7)
    for H, W in median_shapes(K):
        host, dev = strided_view(rng, "float32", 3, H, W)
        want = median_filter(host, size=(1, 3, 3))       # mode="reflect"; planes never mix
        got = run_guarded(lambda out: PP.median3x3(dev, out=out), (3, H, W), torch.float32)
        assert np.array_equal(got, want.view(np.int32)), (H, W)
    assert not np.array_equal(host[0], host[1])           # the planes were distinct


@pytest.mark.parametrize("dtype", DTYPES)
def test_median_mask_equals_scipy(PP, K, dtype):
    rng = np.random.default_rng(8)
    for H, W in median_shapes(K):
        host, dev = strided_view(rng, dtype, 3, H, W)
        if dtype != "float32" and H * W > 16:            # few distinct values: ties everywhere, the threshold value occurs often
            host[...] = host % 7 + (3 if dtype == "uint8" else 300)
            dev.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(DEV))
        smoothed = median_filter(host.astype(np.float32), size=(1, 3, 3))
        thr = float(np.sort(smoothed.ravel())[smoothed.size // 2])   # a value the smoothed planes hold: >= and > differ
        want = (smoothed >= thr).astype(np.uint8)
        assert (smoothed == np.float32(thr)).any() and not np.array_equal(want, (smoothed > thr).astype(np.uint8))
        got = run_guarded(lambda out: PP.median3x3_mask(dev, thr, out=out), (3, H, W), torch.uint8)
        assert np.array_equal(got, want), (dtype, H, W)


def test_median_mask_threshold_is_rounded_to_float32(PP):
    """numpy compares a float32 array with a Python float in float32: 0.1 becomes float32(0.1) > 0.1, and a pixel equal to
    float32(0.1) is foreground"""
    host = np.full((1, 4, 4), np.float32(0.1), dtype=np.float32)
    got = PP.median3x3_mask(torch.from_numpy(host).to(DEV), 0.1).cpu().numpy()
    assert np.array_equal(got, (host >= 0.1).astype(np.uint8)) and got.all()


def test_median_refusals(PP):
    x = torch.zeros((1, 4, 4), dtype=torch.int16, device=DEV)
    with pytest.raises(NotImplementedError):
        PP.median3x3(x)                                    # the fp32 epilogue takes an fp32 source
    with pytest.raises(ValueError):
        PP.median3x3_mask(x, 1.0, out=torch.zeros((1, 4, 4), device=DEV))


# ------------------------------------------------------------------------------------------------ vsx_nan_moments
def moments_sizes(K):
    c = K.MOMENTS_CHUNK
    return [1, c - 1, c, c + 1, 2 * c + 1]


def device_row(values, offset):
    """the values as a float32 device row that starts ``offset`` floats into a 16-byte aligned buffer"""
    buf = torch.empty(values.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    row = buf[offset:offset + values.size]
    row.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
    return row


def moments_twice(PP, row, **kw):
    a, ai = PP.nan_moments(row, **kw)
    b, bi = PP.nan_moments(row, **kw)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), "two runs differ"
    if ai is not None:
        assert torch.equal(ai, bi)
    return a.tolist(), None if ai is None else [int(v) for v in ai.cpu().tolist()]


@pytest.mark.parametrize("offset", [0, 1])   # 0: the float4 path; 1: single loads
def test_moments_float_within_the_summation_bound(PP, K, offset):
    """any fixed order of n float64 additions is within n * 2^-53 * sum |term| of the exact sum (math.fsum's value up to its one
    rounding, which the bound's slack absorbs for n >= 2; for n = 1 the sums are exact)"""
    rng = np.random.default_rng(21)
    for n in moments_sizes(K):
        x = (rng.standard_normal(n) * 50.0 + 20.0).astype(np.float32)
        if n > 2:
            x[[0, n - 1, n // 2]] = np.nan            # NaN first, last and inside
        row = device_row(x, offset)
        ok = x[~np.isnan(x)].astype(np.float64)
        (cnt, vmin, vmax, s), isums = moments_twice(PP, row)
        assert isums is None
        assert cnt == ok.size and vmin == ok.min() and vmax == ok.max()
        assert abs(s - math.fsum(ok)) <= ok.size * U * math.fsum(np.abs(ok)), n
        mean = s / cnt
        (d2, d1, z0, z1), _ = moments_twice(PP, row, mean=mean)
        d = ok - mean                                   # one rounding each, as in the kernel
        assert z0 == 0.0 and z1 == 0.0
        assert abs(d1 - math.fsum(d)) <= ok.size * U * math.fsum(np.abs(d)), n
        want_d2 = float(sum((Fraction(float(v)) ** 2 for v in d), Fraction(0)))   # the terms d^2 are exact inside the kernel's fma
        assert abs(d2 - want_d2) <= ok.size * U * want_d2, n


def test_moments_all_nan(PP, K):
    for n in (1, K.MOMENTS_CHUNK + 1):
        (cnt, vmin, vmax, s), _ = moments_twice(PP, device_row(np.full(n, np.nan, dtype=np.float32), 1))
        assert cnt == 0 and vmin == math.inf and vmax == -math.inf and s == 0.0


def test_moments_integral_sums_are_exact(PP, K):
    rng = np.random.default_rng(22)
    c = K.MOMENTS_CHUNK
    cases = [np.full(2 * c + 1, 65535.0), np.full(c + 1, -32768.0), np.full(1, 65535.0),
             rng.integers(0, 65536, size=3 * c - 5).astype(np.float64), rng.integers(-32768, 32768, size=c).astype(np.float64)]
    for i, x in enumerate(cases):
        row = device_row(x, i % 2)
        (cnt, vmin, vmax, s), isums = moments_twice(PP, row, integral=True)
        xi = [int(v) for v in x]
        assert isums == [sum(xi), sum(v * v for v in xi)], i
        assert cnt == x.size and vmin == x.min() and vmax == x.max() and s == float(sum(xi))   # below 2^53: exact as well


def test_moments_refusals(PP):
    with pytest.raises(RuntimeError):
        PP.nan_moments(torch.zeros(0, device=DEV))
    with pytest.raises(RuntimeError):
        PP.nan_moments(torch.zeros(8, device=DEV)[::2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.nan_moments(torch.zeros(8))


# ------------------------------------------------------------------------------------------------ histograms
def hist_twice(fn):
    a, b = fn().cpu().numpy(), fn().cpu().numpy()
    assert np.array_equal(a, b), "two runs differ"
    return a


def test_hist_int_equals_bincount(PP, K):
    rng = np.random.default_rng(31)
    n = 50_001                                           # more than one workgroup, not a multiple of anything
    lds = K.HIST_LDS_BINS
    cases = [("constant", np.full(n, 1234), 1234, 1),
             ("ends", rng.choice([0, 65535], size=n), 0, 65536),                       # global counters
             ("negative", rng.integers(-32768, -32000, size=n), -32768, 768),          # int16, private counters
             ("lds_limit", rng.integers(5, 5 + lds, size=n), 5, lds),
             ("past_lds_limit", rng.integers(5, 6 + lds, size=n), 5, lds + 1)]
    for name, v, lo, nbins in cases:
        row = device_row(v.astype(np.float32), 1)
        got = hist_twice(lambda: PP.hist_int(row, lo, nbins))
        assert got.dtype == np.int64 and np.array_equal(got, np.bincount(v - lo, minlength=nbins)), name


def test_hist_int_drops_what_is_outside_the_table(PP):
    v = np.array([3, 4, 5, 6, 7, np.nan, -1e20, 1e20, np.inf], dtype=np.float32)
    got = PP.hist_int(device_row(v, 0), 4, 3).cpu().numpy()
    assert got.tolist() == [1, 1, 1]


@pytest.mark.parametrize("nbins", [256, 2, 1024])
def test_hist_edges_equals_np_histogram(PP, nbins):
    rng = np.random.default_rng(32)
    x = (rng.standard_normal(40_000) * 3.0).astype(np.float32)
    e = np.histogram_bin_edges(x, nbins)
    assert e.dtype == np.float32
    x[1000:1000 + min(nbins, 300) + 1] = e[: min(nbins, 300) + 1]    # values exactly on edges, the first and (below) the last among them
    x[5] = e[-1]
    x[6] = e[0]
    want, e2 = np.histogram(x, nbins)
    assert np.array_equal(e, e2)                          # the range did not move
    row = device_row(x, 1)
    got = hist_twice(lambda: PP.hist_edges(row, e))
    assert np.array_equal(got, want) and got.sum() == x.size
    assert np.array_equal(PP.float_hist_edges(float(x.min()), float(x.max()), nbins), e)


def test_hist_edges_drops_outside_and_nan(PP):
    x = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.5, -0.1, np.nan], dtype=np.float32)
    got = PP.hist_edges(device_row(x, 0), np.array([0.0, 1.0, 2.0])).cpu().numpy()
    assert got.tolist() == [2, 3]                         # [0, 1) and [1, 2]: the last bin is closed


# ------------------------------------------------------------------------------------------------ get_val_stats
EXACT_KEYS = ("min", "max", "median", "iqr", "p5", "p95", "p95_p5", "p1", "p99", "p99_p1")


def check_stats(got, arr, n_hint=None):
    """``got`` against the restatement on ``arr``.  min, max and the percentile keys: the same bits.  Integer data: the mean is the
    same exact integer sum divided once, so the same bits; numpy's std is a pairwise two-pass in float64, within
    (log2 n + 8) * 2^-53 relative of the true value, and ours is the exact variance rounded once and a correctly rounded sqrt (well
    inside the 8).  float32 data: numpy's float64-copy mean / std stand for the true values (their own error: (log2 n + 8) * 2^-53
    relative), and a fixed-order float64 sum of n terms is within n * 2^-53 * sum |term| of exact; for the mean that is
    n u mean(|x|), for the variance, a sum of squares, n u var, so n u / 2 relative for the std."""
    want = RP.get_val_stats(arr)
    assert list(got) == list(want) and all(type(v) is float for v in got.values())
    for k in EXACT_KEYS:
        assert got[k].hex() == want[k].hex() or (math.isnan(got[k]) and math.isnan(want[k])), (k, got[k], want[k])
    flat = arr.ravel()
    ok = flat[~np.isnan(flat)] if flat.dtype.kind == "f" else flat
    n = ok.size
    ref_slack = (math.log2(max(n, 2)) + 8) * U
    if flat.dtype.kind != "f":
        assert got["mean"].hex() == want["mean"].hex()
        if not abs(got["std"] - want["std"]) <= ref_slack * want["std"]:
            ints = [int(v) for v in ok]
            var = Fraction(n * sum(v * v for v in ints) - sum(ints) ** 2, n * n)
            true = math.sqrt(var)
            raise AssertionError(f"std: ours {got['std']!r} numpy {want['std']!r} exact-variance sqrt {true!r}: "
                                 f"ours off by {abs(got['std'] - true) / true:.3e}, numpy by {abs(want['std'] - true) / true:.3e}")
        return
    f64 = ok.astype(np.float64)
    mean64, std64 = float(np.mean(f64)), float(np.std(f64))
    assert abs(got["mean"] - mean64) <= n * U * float(np.mean(np.abs(f64))) + ref_slack * abs(mean64)
    assert abs(got["std"] - std64) <= (n * U / 2 + ref_slack) * std64


@pytest.mark.parametrize("case", ["uint16", "uint16_narrow", "float32", "float32_nan", "uint16_one", "float32_one"])
def test_get_val_stats_against_the_restatement(PP, case):
    arr = RP.golden_cases()[case]
    check_stats(PP.get_val_stats(arr), arr)
    dev = torch.from_numpy(arr).to(DEV)
    assert PP.get_val_stats(dev) == PP.get_val_stats(arr)            # a device tensor serves where it is


def test_get_val_stats_larger_rows(PP, K):
    rng = np.random.default_rng(41)
    n = 4 * K.MOMENTS_CHUNK + 3
    u16 = rng.integers(0, 4096, size=n).astype(np.uint16)
    check_stats(PP.get_val_stats(u16), u16)
    f =(rng.standard_normal((n,)) * 12.0 + 90.0).astype(np.float32)
    f[::97] = np.nan
    check_stats(PP.get_val_stats(f), f)
    i16 = rng.integers(-32768, 32768, size=(7, 333)).astype(np.int16)
    check_stats(PP.get_val_stats(i16), i16)
    u8 = rng.integers(0, 256, size=(5000,)).astype(np.uint8)
    check_stats(PP.get_val_stats(u8), u8)


def test_get_val_stats_all_nan_and_refusals(PP):
    got = PP.get_val_stats(np.full((3, 4), np.nan, dtype=np.float32))
    assert list(got) == list(PP.STAT_KEYS) and all(math.isnan(v) for v in got.values())
    with pytest.raises(NotImplementedError):
        PP.get_val_stats(np.zeros(4, dtype=np.float64))
    with pytest.raises(ValueError):
        PP.get_val_stats(np.zeros(0, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ end to end
CHANNELS = ["Phase", "Nuclei"]


def check_meta(got, want, want64, n, integral, where):
    """one statistics dictionary of ``.zattrs`` against the restatement: exact, except mean / std as in check_stats (for float32
    stores ``want64`` is the restatement on the float64 copy of the same sample; the data are positive, so mean |x| is the mean)"""
    assert list(got) == list(want), where
    slack = (math.log2(n) + 8) * U
    for k, v in want.items():
        if k == "mean" and not integral:
            assert abs(got[k] - want64[k]) <= (n * U + slack) * abs(want64[k]), (where, k)
        elif k == "std":
            ref = want[k] if integral else want64[k]
            assert abs(got[k] - ref) <= ((0.0 if integral else n * U / 2) + slack) * ref, (where, k, got[k], ref)
        else:
            assert got[k] == v and type(got[k]) is type(v), (where, k, got[k], v)


def check_store(path, positions, integral, g):
    from viscy_amd.data import open_ome_zarr

    pos64 = {k: v.astype(np.float64) for k, v in positions.items()}
    plate_want, pos_want = RP.normalization_metadata(positions, CHANNELS, -1, g, True, 4)
    plate_w64, pos_w64 = RP.normalization_metadata(pos64, CHANNELS, -1, g, False)
    T, _, Z, Y, X = next(iter(positions.values())).shape
    S, P = Z * -(-Y // g) * -(-X // g), len(positions)
    plate = open_ome_zarr(path, mode="r")
    meta = plate.zattrs["normalization"]
    assert list(meta) == CHANNELS
    for ch in CHANNELS:
        assert list(meta[ch]) == ["dataset_statistics", "timepoint_statistics"]
        check_meta(meta[ch]["dataset_statistics"], plate_want[ch]["dataset_statistics"], plate_w64[ch]["dataset_statistics"], P * T * S,
                   integral, ("plate", ch))
        assert list(meta[ch]["timepoint_statistics"]) == [str(t) for t in range(T)]
        for t in range(T):
            check_meta(meta[ch]["timepoint_statistics"][str(t)], plate_want[ch]["timepoint_statistics"][str(t)],
                       plate_w64[ch]["timepoint_statistics"][str(t)], P * S, integral, ("plate", ch, t))
    thresholds = {}
    for name, pos in plate.positions():
        pm = pos.zattrs["normalization"]
        assert list(pm) == CHANNELS
        for ch in CHANNELS:
            assert list(pm[ch]) == ["dataset_statistics", "fov_statistics", "timepoint_statistics"]
            assert pm[ch]["dataset_statistics"] == meta[ch]["dataset_statistics"]
            check_meta(pm[ch]["fov_statistics"], pos_want[name][ch]["fov_statistics"], pos_w64[name][ch]["fov_statistics"], T * S,
                       integral, (name, ch))
            thresholds[name, ch] = pm[ch]["fov_statistics"]["otsu_threshold"]
            for t in range(T):
                check_meta(pm[ch]["timepoint_statistics"][str(t)], pos_want[name][ch]["timepoint_statistics"][str(t)],
                           pos_w64[name][ch]["timepoint_statistics"][str(t)], S, integral, (name, ch, t))
    return pos_want, thresholds


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_preprocess_end_to_end(PP, tmp_path, dtype):
    from viscy_amd import config
    from viscy_amd.data import open_ome_zarr, write_hcs_plate
    from viscy_amd.data.hcs import HCSDataModule
    from viscy_amd.transforms import NormalizeSampled

    positions = RP.bimodal_plate(dtype)                     # 2 positions, T = 2, 2 channels, Z = 3, 40 x 72
    integral = dtype == "uint16"
    path, path_cli = str(tmp_path / "a.zarr"), str(tmp_path / "cli.zarr")
    for p in (path, path_cli):
        write_hcs_plate(p, positions, CHANNELS)
    PP.generate_normalization_metadata(path, num_workers=2, grid_spacing=8, compute_otsu=True, otsu_grid_spacing=4)
    pos_want, thresholds = check_store(path, positions, integral, 8)
    for (name, ch), thr in thresholds.items():              # background 300 +- 25, blobs 2200 and more above it (float stores: / 7)
        bg = 300.0 if integral else 300.0 / 7.0
        assert bg < thr < 7 * bg, (name, ch, thr)
    PP.generate_fg_masks(path, ["Nuclei"])
    want_masks = RP.fg_masks(positions, CHANNELS, ["Nuclei"], pos_want)
    for name, pos in open_ome_zarr(path, mode="r").positions():
        m = pos["fg_mask"]
        assert m.dtype == np.uint8 and tuple(m.shape) == positions[name].shape and tuple(m.chunks) == (1, 1, 3, 40, 72)
        got = m[slice(None), slice(None), slice(None)]
        assert np.array_equal(got, want_masks[name]), name
        assert (got[:, 0] == 1).all() and 0 < got[:, 1].mean() < 1
    with pytest.raises(FileExistsError):
        PP.generate_fg_masks(path, ["Nuclei"])
    # the command line writes the same attributes and masks
    assert config.main(["preprocess", "--data_path", path_cli, "--block_size", "8", "--compute_otsu", "--otsu_grid_spacing", "4",
                        "--compute_fg_masks", "--fg_mask_channels", "Nuclei", "--num_workers", "2"]) == 0
    a, b = open_ome_zarr(path, mode="r"), open_ome_zarr(path_cli, mode="r")
    assert a.zattrs["normalization"] == b.zattrs["normalization"]
    for (name, pa), (_, pb) in zip(a.positions(), b.positions()):
        assert pa.zattrs["normalization"] == pb.zattrs["normalization"]
        assert np.array_equal(pa["fg_mask"][slice(None), slice(None), slice(None)], pb["fg_mask"][slice(None), slice(None), slice(None)])
    # and the training data path reads what was written: normalisation metadata and the mask next to the target
    dm = HCSDataModule(path, "Phase", "Nuclei", z_window_size=3, batch_size=2, num_workers=0, yx_patch_size=(32, 32), split_ratio=0.5,
                       normalizations=[NormalizeSampled(CHANNELS, "fov_statistics")], fg_mask_key="fg_mask")
    dm.setup("fit")
    batch = next(iter(dm.train_dataloader()))
    assert "fg_mask" in batch and batch["fg_mask"].shape[-2:] == batch["target"].shape[-2:]
    assert set(torch.unique(batch["fg_mask"].float()).tolist()) <= {0.0, 1.0}
    assert float(batch["norm_meta"]["Nuclei"]["fov_statistics"]["mean"][0]) > 0
    from viscy_amd.trainer import Trainer

    dm.training = False                                      # as Trainer does around the hook outside a training step
    out = dm.on_after_batch_transfer(Trainer(seed=None)._to_device(batch), 0)
    src = out["source"].float()                              # (x - fov mean) / fov std over every time point of one FOV
    assert bool(torch.isfinite(src).all()) and abs(float(src.mean())) < 0.5 and 0.5 < float(src.std()) < 2.0
