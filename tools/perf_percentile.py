"""Times the bag-of-channels transforms on one device at the recipes' shapes, event-timed, median of REP runs after WARM
warm-up runs of the same shape, the two sides of each comparison alternating inside one process:

* percentile scaling (``BatchedScaleIntensityRangePercentiles``: radix select + one scale pass) against its own torch
  restatement (``torch.quantile``, which sorts every row, + the tensor expressions) on the same device tensor —
  OPS-1000genes-multimarker-BoC: 512 x (1, 1, 224, 224), lower 1 / upper 99; DynaCLR-2D-MIP-BagOfChannels after its
  augmentations: 256 x (1, 1, 192, 192); and a few long rows, where the select's four passes meet the sort;
* the select alone against ``torch.sort`` of the same rows;
* the fused crop + Z-reduction against ``vsx_crop3d`` followed by ``amax`` — DynaCLR-2D-MIP-BagOfChannels:
  256 x (1, 16, 256, 256) -> window (10, 192, 192).

Prints one JSON line per row.  Usage (GPU box): ``python tools/perf_percentile.py`` (REP / WARM from the environment).
"""

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import transforms as T  # noqa: E402

REP, WARM = int(os.environ.get("REP", 20)), int(os.environ.get("WARM", 3))


def timed(fns: dict) -> dict:
    """median milliseconds of each callable, alternating them run by run"""
    times = {k: [] for k in fns}
    for it in range(WARM + REP):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                times[k].append(e0.elapsed_time(e1))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def torch_percentile(t: T.BatchedScaleIntensityRangePercentiles, img: torch.Tensor) -> torch.Tensor:
    q_low, q_high, b_min, b_max = t._targets()
    B = img.shape[0]
    a_min, a_max = torch.quantile(img.view(B, -1), torch.tensor([q_low, q_high], dtype=img.dtype, device=img.device),
                                  dim=1).reshape(2, B, 1, 1, 1, 1)
    out = (img - a_min) / (a_max - a_min)
    out = out * (b_max - b_min) + b_min
    return out.clip(b_min, b_max)


def main() -> None:
    assert torch.cuda.is_available(), "perf_percentile.py measures on the GPU only"
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, shape in (("OPS multimarker-BoC", (512, 1, 1, 224, 224)), ("2D-MIP BagOfChannels", (256, 1, 1, 192, 192)),
                        ("long rows", (8, 1, 1, 1024, 1024)), ("one row 2^24", (1, 1, 1, 4096, 4096))):
        x = torch.randn(shape, device="cuda", generator=g).abs_() * 300.0 + 100.0     # camera-like: positive, one binade or two
        t = T.BatchedScaleIntensityRangePercentiles(1, 99, 0.0, 1.0, clip=True)
        rows = x.view(shape[0], -1)
        ranks = [r for q in (0.01, 0.99) for r in T.quantile_ranks(q, rows.shape[1])[:2]]
        ms = timed({"transform_ms": lambda: t(x), "torch_quantile_path_ms": lambda: torch_percentile(t, x),
                    "row_select_ms": lambda: T.row_select(rows, ranks), "torch_sort_ms": lambda: torch.sort(rows, dim=1)})
        print(json.dumps({"what": "percentile", "recipe": name, "shape": list(shape), "bytes": x.numel() * 4, **ms}), flush=True)
        del x, rows
    B, crop = 256, (10, 192, 192)
    x = torch.randn((B, 1, 16, 256, 256), device="cuda", generator=g)
    cr = T.BatchedRandSpatialCrop(list(crop))
    cr.generator = torch.Generator().manual_seed(1)
    starts = cr.randomize(x.shape).to("cuda")
    mode = torch.zeros(B, dtype=torch.int32, device="cuda")
    ms = timed({"fused_crop_zreduce_ms": lambda: T.crop_zreduce(x, starts, crop, mode),
                "crop3d_then_amax_ms": lambda: T.crop3d(x, starts, crop).amax(dim=2, keepdim=True)})
    same = torch.equal(T.crop_zreduce(x, starts, crop, mode), T.crop3d(x, starts, crop).amax(dim=2, keepdim=True))
    print(json.dumps({"what": "crop_zreduce", "recipe": "2D-MIP BagOfChannels", "shape": list(x.shape), "window": list(crop),
                      "equal": same, **ms}), flush=True)


if __name__ == "__main__":
    main()
