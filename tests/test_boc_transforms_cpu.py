"""CPU: the bag-of-channels transforms (percentile scaling, random crop, channel-wise Z-reduction) against what the
reference's own classes computed (tests/golden/boc_transforms.pt, tools/gen_golden_boc_transforms.py), the host rank
function against torch.quantile, the YAML seam and the crop -> Z-reduction peephole."""

import warnings

import pytest
import torch

from tests.conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("boc_transforms.pt")


def test_percentile_scaling_equals_the_reference(gold):
    from viscy_amd.transforms import BatchedScaleIntensityRangePercentiles, BatchedScaleIntensityRangePercentilesd

    p = gold["percentile"]
    seen = set()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # the degenerate branch warns on the host path, as the reference does
        for case in p["cases"]:
            kw = case["kwargs"]
            y = BatchedScaleIntensityRangePercentiles(**kw)(p[case["input"]].clone())
            assert torch.equal(y, case["y"]), (kw, case["input"])
            seen.add((bool(kw.get("clip")), bool(kw.get("relative")), bool(kw.get("channel_wise")), case["input"]))
        d = BatchedScaleIntensityRangePercentilesd(["a", "b"], lower=1, upper=99, b_min=0.0, b_max=1.0, clip=True,
                                                   allow_missing_keys=True)({"a": p["x"].clone(), "other": p["x_const"]})
    assert torch.equal(d["a"], p["dict_a"]) and d["other"] is p["x_const"]
    # clip on / off, relative, channel_wise, and the batch with one constant row all took part
    for want in ((True, False, False, "x"), (False, False, False, "x"), (True, True, False, "x"), (True, False, True, "x"),
                 (True, False, False, "x_const"), (True, False, True, "x_const_ch")):
        assert want in seen, want
    # the degenerate branch is batch-wide: with one constant sample every sample is only shifted
    first = p["cases"][0]
    assert first["input"] == "x" and p["cases"][1]["input"] == "x_const"
    assert torch.equal(p["cases"][1]["y"][0], p["x_const"][0] - torch.quantile(p["x_const"][0].flatten(), 0.01) + 0.0)
    with pytest.raises(KeyError):
        BatchedScaleIntensityRangePercentilesd(["a", "b"], 1, 99, 0.0, 1.0)({"a": p["x"].clone()})
    with pytest.raises(ValueError, match="relative"):
        BatchedScaleIntensityRangePercentiles(1, 99, None, 1.0, relative=True)(p["x"].clone())


@pytest.mark.parametrize("n", [1, 2, 5, 101, 4097, 10001])
def test_quantile_ranks_are_torch_quantiles(n):
    """(lo, hi, w) from the shape alone select what torch.quantile interpolates: on sorted ramps (a linear one, where the value
    is the fractional rank itself, and a quadratic one, where a wrong neighbour shows) the lerp of the two picks is bit-equal"""
    from viscy_amd.transforms import quantile_ranks

    i = torch.arange(n, dtype=torch.float32)
    for ramp in (i, i * i * 0.25 - 3.0):
        for q in (0.0, 0.01, 0.05, 0.5, 0.95, 0.99, 0.999, 1.0, 1 / 100.0, 50 / 100.0, 99 / 100.0):
            lo, hi, w = quantile_ranks(q, n)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= w < 1.0
            want = torch.quantile(ramp, torch.tensor(q, dtype=torch.float32))
            got = torch.lerp(ramp[lo], ramp[hi], torch.tensor(w))
            assert torch.equal(got, want), (n, q, lo, hi, w, got, want)
            if w == 0.0:
                assert torch.equal(ramp[lo], want)
    if n == 10001:   # the shape the GPU test leans on: n - 1 = 10000 makes the 1 % and 99 % ranks integral
        assert quantile_ranks(0.01, n) == (100, 100, 0.0) and quantile_ranks(0.99, n) == (9900, 9900, 0.0)


def test_z_reduction_equals_the_reference(gold):
    from viscy_amd.transforms import BatchedChannelWiseZReduction, BatchedChannelWiseZReductiond

    z = gold["zreduce"]
    v, v_nan, mask = z["x"], z["x_nan"], z["mask"]
    assert torch.equal(BatchedChannelWiseZReduction("mip")(v.clone()), z["mip"])
    assert torch.equal(BatchedChannelWiseZReduction("center")(v.clone()), z["center"])
    assert torch.equal(BatchedChannelWiseZReduction()(v.clone(), is_labelfree=mask), z["mixed"])
    got = BatchedChannelWiseZReduction()(v_nan.clone(), is_labelfree=mask)
    assert torch.equal(got.isnan(), z["mixed_nan"].isnan()) and got.isnan().sum() == 1
    assert torch.equal(got.nan_to_num(7.0), z["mixed_nan"].nan_to_num(7.0))
    assert torch.equal(BatchedChannelWiseZReduction("mip")(v[:, :, :2].clone()), z["z2_mip"])
    assert torch.equal(BatchedChannelWiseZReduction("center")(v[:, :, :2].clone()), z["z2_center"])
    one = v[:, :, :1].clone()
    assert BatchedChannelWiseZReduction()(one) is one                        # Z == 1 passes through
    d = {"a": v.clone(), "_is_labelfree": mask}
    out = BatchedChannelWiseZReductiond(["a", "b"], allow_missing_keys=True)(d)
    assert "_is_labelfree" not in out and torch.equal(out["a"], z["dict_boc_a"])
    out = BatchedChannelWiseZReductiond(["a", "b"], labelfree_keys=["b"])({"a": v.clone(), "b": v_nan.clone(), "_is_labelfree": mask})
    assert torch.equal(out["a"], z["dict_all_a"])
    assert torch.equal(out["b"].nan_to_num(7.0), z["dict_all_b"].nan_to_num(7.0))
    with pytest.raises(ValueError, match="default_strategy"):
        BatchedChannelWiseZReduction("mean")
    with pytest.raises(ValueError, match="default_strategy"):
        BatchedChannelWiseZReductiond(["a"], default_strategy="max")
    with pytest.raises(KeyError):
        BatchedChannelWiseZReductiond(["a", "b"])({"a": v.clone()})


def test_crop_gather_equals_the_reference_and_draws_stay_inside(gold):
    from viscy_amd.transforms import BatchedRandSpatialCrop, BatchedRandSpatialCropd

    c = gold["crop"]
    x, size, starts = c["x"], tuple(c["size"]), c["starts"]
    assert torch.equal(BatchedRandSpatialCrop(list(size))(x.clone(), params=starts), c["y"])
    # one draw per sample, shared by the keys
    t = BatchedRandSpatialCropd(["a", "b"], roi_size=list(size))
    t.cropper.generator = torch.Generator().manual_seed(5)
    out = t({"a": x.clone(), "b": x.clone() * 2.0, "other": 1})
    assert out["a"].shape == (2, 2) + size and torch.equal(out["b"], out["a"] * 2.0) and out["other"] == 1
    out = t({"a": x.clone(), "b": x.clone()}, params=starts)
    assert torch.equal(out["a"], c["y"]) and torch.equal(out["b"], c["y"])
    # every start is inside [0, dim - size], both ends are reached, samples differ
    cr = BatchedRandSpatialCrop([3, 4, 6])
    cr.generator = torch.Generator().manual_seed(0)
    st = cr.randomize((512, 1, 5, 7, 9))
    assert st.shape == (512, 3) and st.dtype == torch.long
    for d, hi in enumerate((2, 3, 3)):
        assert st[:, d].min() == 0 and st[:, d].max() == hi
    # the centre crop, an int roi, entries that keep or exceed the axis
    ctr = BatchedRandSpatialCrop([3, 4, 6], random_center=False)
    assert ctr.randomize((2, 1, 5, 7, 9)).tolist() == [[1, 1, 1]] * 2
    assert BatchedRandSpatialCrop(4)(x.clone()).shape == (2, 2, 4, 4, 4)
    assert BatchedRandSpatialCrop([-1, 100, 6])(x.clone()).shape == (2, 2, 5, 7, 6)
    with pytest.raises(ValueError, match="random size"):
        BatchedRandSpatialCrop([3, 4, 6], random_size=True)
    with pytest.raises(ValueError, match="random size"):
        BatchedRandSpatialCropd(["a"], [3, 4, 6], random_size=True)
    with pytest.raises(ValueError, match="3D"):
        BatchedRandSpatialCrop([4, 6])(x[:, :, 0].clone())
    with pytest.raises(ValueError, match="3D"):
        BatchedRandSpatialCropd(["a"], [3, 4, 6])({"a": x[:, :, 0].clone()})
    with pytest.raises(KeyError):
        BatchedRandSpatialCropd(["a", "b"], [3, 4, 6])({"a": x.clone()})


def test_class_map_resolves_the_recipe_names():
    from viscy_amd import transforms as T
    from viscy_amd.config import CLASS_MAP, instantiate

    for name in ("BatchedScaleIntensityRangePercentiles", "BatchedScaleIntensityRangePercentilesd", "BatchedRandSpatialCrop",
                 "BatchedRandSpatialCropd", "BatchedChannelWiseZReduction", "BatchedChannelWiseZReductiond"):
        assert CLASS_MAP[f"viscy_transforms.{name}"] == f"viscy_amd.transforms.{name}"
    # the entries as the recipes write them (2-D MIP bag-of-channels and OPS)
    chain = instantiate([
        {"class_path": "viscy_transforms.BatchedScaleIntensityRangePercentilesd",
         "init_args": {"keys": ["channel_0"], "lower": 50, "upper": 99, "b_min": 0.0, "b_max": 1.0, "clip": True}},
        {"class_path": "viscy_transforms.BatchedRandSpatialCropd", "init_args": {"keys": ["channel_0"], "roi_size": [10, 192, 192]}},
        {"class_path": "viscy_transforms.BatchedChannelWiseZReductiond", "init_args": {"keys": ["channel_0"], "allow_missing_keys": True}},
    ])
    assert [type(t) for t in chain] == [T.BatchedScaleIntensityRangePercentilesd, T.BatchedRandSpatialCropd,
                                        T.BatchedChannelWiseZReductiond]
    assert chain[0].scaler.lower == 50 and chain[1].cropper.roi_size == [10, 192, 192] and chain[2].allow_missing_keys
    # ... and a data module built from a recipe tree that names them composes the chain, crop and Z-reduction as one gather
    dm = instantiate({"class_path": "viscy_data.hcs.HCSDataModule", "init_args": {
        "data_path": "plate.zarr", "source_channel": "Phase3D", "target_channel": ["Nuclei"], "z_window_size": 10, "batch_size": 4,
        "gpu_augmentations": [
            {"class_path": "viscy_transforms.BatchedScaleIntensityRangePercentilesd",
             "init_args": {"keys": ["source"], "lower": 1, "upper": 99, "b_min": 0.0, "b_max": 1.0, "clip": True}},
            {"class_path": "viscy_transforms.BatchedRandSpatialCropd", "init_args": {"keys": ["source"], "roi_size": [10, 192, 192]}},
            {"class_path": "viscy_transforms.BatchedChannelWiseZReductiond", "init_args": {"keys": ["source"], "allow_missing_keys": True}}]}})
    assert [type(t) for t in dm._gpu_augmentations.transforms] == [T.BatchedScaleIntensityRangePercentilesd, T._CropThenZReduce]


def test_crop_then_z_reduction_is_fused_only_when_adjacent(gold):
    from viscy_amd import transforms as T

    c = gold["crop"]

    def parts():
        crop = T.BatchedRandSpatialCropd(["a"], roi_size=list(c["size"]))
        return crop, T.BatchedRandFlipd(["a"], prob=0.0), T.BatchedChannelWiseZReductiond(["a"], allow_missing_keys=True)

    crop, flip, zred = parts()
    fused = T.fuse_crop_zreduce([crop, zred])
    assert len(fused) == 1 and isinstance(fused[0], T._CropThenZReduce) and fused[0].crop is crop and fused[0].zreduce is zred
    apart = [crop, flip, zred]
    assert T.fuse_crop_zreduce(apart) == apart
    other_keys = [crop, T.BatchedChannelWiseZReductiond(["b"])]
    assert T.fuse_crop_zreduce(other_keys) == other_keys
    assert T.fuse_crop_zreduce([zred, crop]) == [zred, crop]
    # on the host the fused object is the two transforms one after the other
    out = fused[0]({"a": c["x"].clone()}, params=c["starts"])
    assert torch.equal(out["a"], c["y_mip"])
    out = fused[0]({"a": c["x"].clone(), "_is_labelfree": torch.tensor([True, False])}, params=c["starts"])
    assert torch.equal(out["a"], c["y_mixed"]) and "_is_labelfree" not in out
    # same draws as the pair: the fused call consumes the crop's generator once
    crop.cropper.generator = torch.Generator().manual_seed(3)
    a = fused[0]({"a": c["x"].clone()})["a"]
    crop.cropper.generator = torch.Generator().manual_seed(3)
    b = zred(crop({"a": c["x"].clone()}))["a"]
    assert torch.equal(a, b)


def test_device_only_entry_points_refuse_cpu_tensors():
    from viscy_amd import transforms as T

    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        T.row_select(x, (0, 7))
    with pytest.raises(RuntimeError, match="no CPU"):
        T.percentile_scale(x, torch.zeros(2), torch.ones(2), torch.zeros(2), 0.0, 1.0, True)
    with pytest.raises(RuntimeError, match="no CPU"):
        T.crop_zreduce(torch.zeros(1, 1, 2, 3, 4), None, (2, 3, 4), torch.zeros(1))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """sizes and ranks outside the contract are a VSX_CHECK error: nothing is launched, so this runs without a device (the
    pointers are host arrays that no kernel ever sees)"""
    import ctypes

    from viscy_amd import _lib

    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    ws = (ctypes.c_uint32 * 4096)()
    p, w = ctypes.addressof(buf), ctypes.addressof(ws)
    ranks = lambda *r: (ctypes.c_int64 * max(len(r), 1))(*r)  # noqa: E731
    assert l.vsx_row_select_ws_bytes(3, 4) == 4 * (3 * 4 * 258 + 3)
    assert l.vsx_row_select_ws_bytes(0, 4) == 0 and l.vsx_row_select_ws_bytes(1, 5) == 0
    for args, msg in (((p, p, w, 16384, 0, 8, ranks(0), 1, None), b"rows >= 1"),
                      ((p, p, w, 16384, 1, 0, ranks(0), 1, None), b"1 <= n"),
                      ((p, p, w, 16384, 1, 1 << 31, ranks(0), 1, None), b"2^31 - 1"),
                      ((p, p, w, 16384, 1, 8, ranks(8), 1, None), b"rank 8 outside [0, 8)"),
                      ((p, p, w, 16384, 1, 8, ranks(-1), 1, None), b"rank -1 outside"),
                      ((p, p, w, 16384, 1, 8, ranks(0, 1, 2, 3, 4), 5, None), b"1 to 4 ranks"),
                      ((p, p, w, 16384, 1, 8, ranks(), 0, None), b"1 to 4 ranks"),
                      ((p, p, w, 16, 1, 8, ranks(0, 7), 2, None), b"workspace of 16 bytes, 2068 needed"),
                      ((None, p, w, 16384, 1, 8, ranks(0), 1, None), b"null argument")):
        assert l.vsx_row_select(*args) == 1 and msg in l.vsx_last_error(), (args[4:8], l.vsx_last_error())
    assert l.vsx_percentile_scale(p, p, p, p, p, 2, 4, 0.0, 1.0, 16, None) == 1 and b"4-bit mask" in l.vsx_last_error()
    assert l.vsx_percentile_scale(p, p, p, p, p, 0, 4, 0.0, 1.0, 1, None) == 1
    assert l.vsx_percentile_scale(p, p, p, p, p, 1 << 40, 1 << 40, 0.0, 1.0, 1, None) == 1 and b"overflows" in l.vsx_last_error()
    assert l.vsx_crop_zreduce(p, p, None, p, 1, 1, 2, 2, 2, 3, 2, 2, None) == 1 and b"window (3,2,2) in (2,2,2)" in l.vsx_last_error()
    assert l.vsx_crop_zreduce(p, p, None, None, 1, 1, 2, 2, 2, 2, 2, 2, None) == 1
