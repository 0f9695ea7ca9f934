"""CPU: the host side of ``viscy_amd.preprocess`` — the restatement against the reference's recorded get_val_stats, numpy's
percentile interpolation from exact order statistics, the Otsu scan, ``write_meta_field``, the ``preprocess`` command line and the
refusals that come before a device is needed."""

import json
import os
import warnings

import numpy as np
import pytest

from tests import ref_preprocess as RP
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "preprocess_stats.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ restatement == reference
def test_restatement_equals_the_reference_bit_for_bit(golden):
    assert golden["numpy"] == np.__version__, "the golden holds numpy's own float32 means and interpolation: regenerate it"
    cases = RP.golden_cases()
    assert set(cases) == set(golden["stats"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, arr in cases.items():
            row = RP.get_val_stats(arr)
            assert list(row) == golden["keys"], name
            for k, v in row.items():
                assert type(v) is float
                assert v.hex() == golden["stats"][name][k], (name, k, v, float.fromhex(golden["stats"][name][k]))


def test_module_key_order_is_the_reference_order(golden):
    from viscy_amd import preprocess as PP

    assert list(PP.STAT_KEYS) == golden["keys"]
    assert list(PP._stats_dict(0.0, 1.0, 0.5, 0.1, range(7))) == golden["keys"]
    assert list(PP.PERCENTILES) == RP.PERCENTILES


# ------------------------------------------------------------------------------------------------ percentiles
def _percentiles_via_order_stats(arr):
    from viscy_amd import preprocess as PP

    flat = arr.ravel()
    if flat.dtype.kind == "f":
        flat = flat[~np.isnan(flat)]
    s = np.sort(flat)
    lo, hi, gamma = PP.percentile_ranks(s.size)
    return PP.percentiles_from_order_stats(s[lo], s[hi], gamma)


@pytest.mark.parametrize("dtype", ["uint16", "int16", "uint8", "float32"])
@pytest.mark.parametrize("n", [1, 2, 3, 100, 101, 4999, 65537])
def test_percentiles_from_order_stats_equal_numpy(dtype, n):
    rng = np.random.default_rng(n * 7 + len(dtype))
    if dtype == "float32":
        arr = (rng.standard_normal(n) * 1e3).astype(np.float32)
    else:
        info = np.iinfo(dtype)
        arr = rng.integers(info.min, info.max + 1, size=n).astype(dtype)
    want = np.nanpercentile(arr, RP.PERCENTILES)
    got = _percentiles_via_order_stats(arr)
    assert want.dtype == np.float64 and got.dtype == np.float64
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


def test_percentiles_with_nans_equal_nanpercentile():
    arr = RP.golden_cases()["float32_nan"]
    want = np.nanpercentile(arr, RP.PERCENTILES)
    got = _percentiles_via_order_stats(arr)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_percentile_ranks_are_inside_the_row():
    from viscy_amd import preprocess as PP

    for n in (1, 2, 7, 100, 2 ** 31 - 1):
        lo, hi, gamma = PP.percentile_ranks(n)
        assert all(0 <= a <= b < n and b - a <= 1 for a, b in zip(lo, hi)), n
        assert gamma.dtype == np.float64 and len(lo) == len(hi) == 7


# ------------------------------------------------------------------------------------------------ Otsu
def test_otsu_separates_a_bimodal_histogram():
    from viscy_amd.preprocess import otsu_from_histogram

    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(90, 131, 6000), rng.integers(2900, 3101, 2500)]).astype(np.uint16)
    thr = otsu_from_histogram(*RP.otsu_histogram(x))
    assert type(thr) is float and 130 <= thr < 2900
    # the definition, evaluated the slow way: the integer threshold that maximises the inter-class variance, first maximum
    best, arg = -1.0, None
    for k in range(int(x.min()), int(x.max())):
        a, b = x[x <= k].astype(np.float64), x[x > k].astype(np.float64)
        v = a.size * b.size * (a.mean() - b.mean()) ** 2
        if v > best * (1 + 1e-12):
            best, arg = v, k
    assert thr == float(arg)
    xf = np.concatenate([rng.normal(1.0, 0.1, 5000), rng.normal(9.0, 0.3, 3000)]).astype(np.float32)
    thr = otsu_from_histogram(*RP.otsu_histogram(xf))
    # across the empty gap the variance is flat: the first maximum is the bin that holds the lower mode's largest value
    width = (float(xf.max()) - float(xf.min())) / 256
    assert bool((xf[:5000] <= thr + width).all()) and bool((xf[5000:] > thr + width).all())


def test_otsu_of_a_constant_is_the_constant():
    from viscy_amd.preprocess import otsu_from_histogram

    assert otsu_from_histogram([1234], [77]) == 77.0
    assert RP.otsu_threshold(np.full((2, 3, 5, 6), 412, dtype=np.uint16)) == 412.0
    assert RP.otsu_threshold(np.full((1, 1, 4, 4), -2.5, dtype=np.float32)) == -2.5
    with pytest.raises(ValueError):
        otsu_from_histogram([1, 2], [1.0])


def test_float_hist_edges_are_numpys():
    from viscy_amd.preprocess import float_hist_edges

    x = (np.random.default_rng(5).standard_normal(4000) * 3).astype(np.float32)
    _, e = np.histogram(x, 256)
    mine = float_hist_edges(float(x.min()), float(x.max()))
    assert mine.dtype == e.dtype == np.float32 and np.array_equal(mine, e)


# ------------------------------------------------------------------------------------------------ stores
def _plate(tmp_path, dtype=np.uint16, norm_meta=None):
    from viscy_amd.data import open_ome_zarr, write_hcs_plate

    pos = RP.bimodal_plate(dtype, shape=(2, 2, 1, 12, 16))
    path = str(tmp_path / "plate.zarr")
    write_hcs_plate(path, pos, ["Phase", "Nuclei"], norm_meta=norm_meta)
    return path, open_ome_zarr(path, mode="r+")


def test_write_meta_field_three_merge_cases(tmp_path):
    from viscy_amd.data import open_ome_zarr
    from viscy_amd.preprocess import write_meta_field

    path, plate = _plate(tmp_path)
    _, pos = next(iter(plate.positions()))
    for node in (plate, pos):
        kept = {k: v for k, v in node.zattrs.items() if k != "normalization"}
        write_meta_field(node, {"a": 1}, "normalization", "Phase")                  # no field yet
        assert node.zattrs["normalization"] == {"Phase": {"a": 1}}
        write_meta_field(node, {"b": 2}, "normalization", "Nuclei")                 # field, new subfield
        assert node.zattrs["normalization"] == {"Phase": {"a": 1}, "Nuclei": {"b": 2}}
        write_meta_field(node, {"a": 3, "c": 4}, "normalization", "Phase")          # subfield updated key by key
        assert node.zattrs["normalization"] == {"Phase": {"a": 3, "c": 4}, "Nuclei": {"b": 2}}
        assert {k: v for k, v in node.zattrs.items() if k != "normalization"} == kept
    again = open_ome_zarr(path, mode="r")                                           # and it is on disk
    assert again.zattrs["normalization"]["Phase"] == {"a": 3, "c": 4} and "plate" in again.zattrs
    assert next(iter(again.positions()))[1].zattrs["normalization"]["Nuclei"] == {"b": 2}


def test_fg_masks_refusals_come_before_the_device(tmp_path):
    from viscy_amd.preprocess import generate_fg_masks

    path, plate = _plate(tmp_path, norm_meta={"Nuclei": {"fov_statistics": {"otsu_threshold": 500.0}},
                                              "Phase": {"fov_statistics": {"mean": 1.0}}})
    with pytest.raises(KeyError, match="otsu_threshold"):
        generate_fg_masks(path, ["Phase"])
    with pytest.raises(ValueError):
        generate_fg_masks(path, ["NoSuchChannel"])
    _, pos = next(iter(plate.positions()))
    assert "fg_mask" not in pos                                                     # a refusal leaves nothing behind
    pos.create_zeros("fg_mask", (2, 2, 1, 12, 16), np.uint8)
    with pytest.raises(FileExistsError, match="fg_mask"):
        generate_fg_masks(path, ["Nuclei"])
    generate_fg_masks_other_key_needs_the_device(path)


def generate_fg_masks_other_key_needs_the_device(path):
    import torch

    from viscy_amd.preprocess import generate_fg_masks, generate_normalization_metadata

    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        generate_fg_masks(path, ["Nuclei"], fg_mask_key="other")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        generate_normalization_metadata(path)


# ------------------------------------------------------------------------------------------------ Trainer and command line
def test_trainer_preprocess_refuses_masks_without_otsu(tmp_path):
    from viscy_amd.trainer import Trainer

    path, _ = _plate(tmp_path)
    with pytest.raises(ValueError, match="compute_fg_masks requires compute_otsu=True"):
        Trainer(seed=None).preprocess(path, compute_fg_masks=True)


def test_cli_parses_preprocess_without_config(monkeypatch, tmp_path):
    from viscy_amd import config, trainer

    seen = {}
    monkeypatch.setattr(trainer.Trainer, "preprocess", lambda self, **kw: seen.update(kw))
    assert config.main(["preprocess", "--data_path", "p.zarr"]) == 0
    assert seen == dict(data_path="p.zarr", channel_names=-1, num_workers=1, block_size=32, compute_otsu=False, otsu_grid_spacing=8,
                        compute_fg_masks=False, fg_mask_channels=None, fg_mask_key="fg_mask")
    seen.clear()
    assert config.main(["preprocess", "--data_path", "p.zarr", "--channel_names", "Phase", "Nuclei", "--block_size", "16",
                        "--compute_otsu", "--compute_fg_masks", "true", "--fg_mask_channels", "Nuclei", "--num_workers", "4",
                        "--otsu_grid_spacing", "4", "--fg_mask_key", "m"]) == 0
    assert seen == dict(data_path="p.zarr", channel_names=["Phase", "Nuclei"], num_workers=4, block_size=16, compute_otsu=True,
                        otsu_grid_spacing=4, compute_fg_masks=True, fg_mask_channels=["Nuclei"], fg_mask_key="m")
    with pytest.raises(SystemExit):
        config.main(["preprocess"])                                                 # --data_path is required


@pytest.mark.parametrize("sub", ["fit", "predict", "test"])
def test_cli_still_requires_config_for_the_recipe_stages(sub):
    from viscy_amd import config

    with pytest.raises(SystemExit) as e:
        config.main([sub])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        config.parser().parse_args(["preprocess", "--config", "x.yml"])             # the recipe parser does not know the stage


def test_header_declares_the_preprocess_kernels():
    from viscy_amd import _lib

    for name in ("vsx_grid_sample", "vsx_median3x3", "vsx_nan_moments", "vsx_nan_moments_ws_bytes", "vsx_hist_int", "vsx_hist_edges"):
        assert name in _lib.exported_symbols()
    assert _lib.MEDIAN_COLS == 62 and _lib.MOMENTS_CHUNK % 1024 == 0 and _lib.MOMENTS_PART_BYTES == 48
