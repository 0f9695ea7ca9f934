"""Writes tests/golden/boc_transforms.pt: what the reference's own ``BatchedScaleIntensityRangePercentiles``,
``BatchedChannelWiseZReduction(d)`` and the gather of ``BatchedRandSpatialCrop`` compute on small seeded inputs.

The reference modules (``viscy_transforms/_percentile_scale.py``, ``_z_reduction.py``, ``_crop.py``) are loaded from a checkout
of the reference and run on stub ``monai.transforms`` classes that carry only what those modules touch: constructor
attributes and the key iteration of ``MapTransform``.  MONAI's random stream is not reproduced: the crop is called with
``randomize=False`` and injected ``_batch_slices``, so only its gather is recorded.

Usage: ``python tools/gen_golden_boc_transforms.py [--reference /path/to/reference]`` (default: $VISCY_REFERENCE or
/root/reference).  Nothing of the reference is copied: the file holds inputs, keyword sets and outputs.
"""

import argparse
import importlib.util
import os
import sys
import types
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "boc_transforms.pt")


def _stub_monai():
    class MapTransform:
        def __init__(self, keys, allow_missing_keys=False):
            self.keys = (keys,) if isinstance(keys, str) else tuple(keys)
            self.allow_missing_keys = allow_missing_keys

        def key_iterator(self, data):
            for k in self.keys:
                if k in data:
                    yield k
                elif not self.allow_missing_keys:
                    raise KeyError(k)

        def first_key(self, data):
            return next(iter(self.key_iterator(data)), ())

    class ScaleIntensityRangePercentiles:
        def __init__(self, lower, upper, b_min, b_max, clip=False, relative=False, channel_wise=False, dtype=None):
            self.lower, self.upper, self.b_min, self.b_max = lower, upper, b_min, b_max
            self.clip, self.relative, self.channel_wise, self.dtype = clip, relative, channel_wise, dtype

    class RandSpatialCrop:
        def __init__(self, roi_size, max_roi_size=None, random_center=True, random_size=False, lazy=False):
            self.roi_size, self.max_roi_size = roi_size, max_roi_size
            self.random_center, self.random_size = random_center, random_size
            self._size = None

    class CenterSpatialCrop:
        def __init__(self, roi_size, lazy=False):
            self.roi_size = roi_size

    class Cropd(MapTransform):
        def __init__(self, keys, cropper, allow_missing_keys=False, lazy=False):
            super().__init__(keys, allow_missing_keys)
            self.cropper = cropper

    class RandCropd(Cropd):
        pass

    monai = types.ModuleType("monai")
    mt = types.ModuleType("monai.transforms")
    for c in (MapTransform, ScaleIntensityRangePercentiles, RandSpatialCrop, CenterSpatialCrop, Cropd, RandCropd):
        setattr(mt, c.__name__, c)
    monai.transforms = mt
    sys.modules["monai"], sys.modules["monai.transforms"] = monai, mt


def _load(name: str, path: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


PERCENTILE_CASES = [
    dict(lower=1, upper=99, b_min=0.0, b_max=1.0, clip=True),                      # the OPS recipes
    dict(lower=50, upper=99, b_min=0.0, b_max=1.0, clip=True),
    dict(lower=1, upper=99, b_min=0.0, b_max=1.0, clip=False),
    dict(lower=5, upper=95, b_min=None, b_max=None, clip=False),
    dict(lower=2, upper=98, b_min=-1.0, b_max=3.0, clip=True, relative=True),
    dict(lower=1, upper=99, b_min=0.0, b_max=1.0, clip=True, channel_wise=True),
    dict(lower=10, upper=90, b_min=0.5, b_max=2.0, clip=False, relative=True, channel_wise=True),
]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VISCY_REFERENCE", "/root/reference"))
    src = os.path.join(ap.parse_args().reference, "packages", "viscy-transforms", "src", "viscy_transforms")
    _stub_monai()
    sys.modules["viscy_transforms"] = types.ModuleType("viscy_transforms")
    ps = _load("viscy_transforms._percentile_scale", os.path.join(src, "_percentile_scale.py"))
    zr = _load("viscy_transforms._z_reduction", os.path.join(src, "_z_reduction.py"))
    cr = _load("viscy_transforms._crop", os.path.join(src, "_crop.py"))

    g = torch.Generator().manual_seed(2024)
    gold: dict = {}
    # ---- percentile scaling: (3, 2, 2, 5, 7) = 140 values per sample, 70 per (sample, channel): no rank is integral
    x = torch.randn((3, 2, 2, 5, 7), generator=g) * 7.0 + 3.0
    x_const = x.clone()
    x_const[1] = 2.5                     # one constant sample: a_min == a_max there -> the batch-wide degenerate branch
    x_const_ch = x.clone()
    x_const_ch[2, 1] = -4.0              # one constant (sample, channel): degenerate for channel 1 only when channel_wise
    cases = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, kw in enumerate(PERCENTILE_CASES):
            for tag, inp in (("x", x), ("x_const", x_const), ("x_const_ch", x_const_ch)):
                if (tag == "x_const" and i not in (0, 3, 4, 5)) or (tag == "x_const_ch" and not kw.get("channel_wise")):
                    continue
                cases.append({"kwargs": dict(kw), "input": tag, "y": ps.BatchedScaleIntensityRangePercentiles(**kw)(inp.clone())})
        d = ps.BatchedScaleIntensityRangePercentilesd(["a", "b"], lower=1, upper=99, b_min=0.0, b_max=1.0, clip=True,
                                                     allow_missing_keys=True)({"a": x.clone(), "other": x_const.clone()})
    gold["percentile"] = {"x": x, "x_const": x_const, "x_const_ch": x_const_ch, "cases": cases, "dict_a": d["a"]}

    # ---- Z reduction
    v = torch.randn((3, 2, 5, 5, 6), generator=g)
    v_nan = v.clone()
    v_nan[1, 0, 3, 2, 4] = float("nan")
    mask = torch.tensor([True, False, True])
    z = {"x": v, "x_nan": v_nan, "mask": mask,
         "mip": zr.BatchedChannelWiseZReduction("mip")(v.clone()),
         "center": zr.BatchedChannelWiseZReduction("center")(v.clone()),
         "mixed": zr.BatchedChannelWiseZReduction("mip")(v.clone(), is_labelfree=mask),
         "mixed_nan": zr.BatchedChannelWiseZReduction("mip")(v_nan.clone(), is_labelfree=mask),
         "z2_mip": zr.BatchedChannelWiseZReduction("mip")(v[:, :, :2].clone()),
         "z2_center": zr.BatchedChannelWiseZReduction("center")(v[:, :, :2].clone())}
    boc = zr.BatchedChannelWiseZReductiond(["a", "b"], allow_missing_keys=True)({"a": v.clone(), "_is_labelfree": mask})
    assert "_is_labelfree" not in boc
    z["dict_boc_a"] = boc["a"]
    allch = zr.BatchedChannelWiseZReductiond(["a", "b"], labelfree_keys=["b"])({"a": v.clone(), "b": v_nan.clone(), "_is_labelfree": mask})
    z["dict_all_a"], z["dict_all_b"] = allch["a"], allch["b"]
    gold["zreduce"] = z

    # ---- the crop's gather at injected window starts
    c = torch.randn((2, 2, 5, 7, 9), generator=g)
    size, starts = (3, 4, 6), [[0, 0, 0], [2, 3, 3]]
    t = cr.BatchedRandSpatialCrop(roi_size=list(size))
    t._batch_slices = [tuple(slice(s, s + n) for s, n in zip(st, size)) for st in starts]
    gold["crop"] = {"x": c, "size": size, "starts": torch.tensor(starts), "y": t(c.clone(), randomize=False)}
    # crop -> Z reduction, the tail of the 2-D MIP recipes
    gold["crop"]["y_mip"] = zr.BatchedChannelWiseZReduction("mip")(gold["crop"]["y"].clone())
    gold["crop"]["y_mixed"] = zr.BatchedChannelWiseZReduction("mip")(gold["crop"]["y"].clone(), is_labelfree=torch.tensor([True, False]))

    torch.save(gold, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
