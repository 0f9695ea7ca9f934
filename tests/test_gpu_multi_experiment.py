"""GPU: the multi-experiment DynaCLR feed end to end.  The golden table (tests/golden/multi_experiment.pt) over the synthetic
two-experiment stores: batches formed on the device by vsx_patch_gather_scaled out of the frame cache carry the bits of the
host path (which tests/test_multi_experiment_cpu.py pins to the reference's recorded patches), with a budget that holds every
frame, one that holds one frame (eviction, never of a frame the batch needs) and none (everything host-gathered through the same
launch).  Then ContrastiveModule takes a fit step on batches of MultiExperimentDataModule through Trainer.fit."""

import numpy as np
import pytest
import torch

from tests import multi_experiment_cases as cases
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
FRAME_BYTES = {name: len(s["channels"]) * s["Z"] * s["H"] * s["W"] * np.dtype(s["dtype"]).itemsize for name, s in cases.STORES.items()}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from viscy_amd.data import multi_experiment as me

    golden = load_golden("multi_experiment.pt")
    root = tmp_path_factory.mktemp("multi_experiment_gpu")
    cases.write_stores(root)
    parquet = str(root / "cells.parquet")
    me.write_cell_index(cases.table_frame(golden["table"], root), parquet)
    registry, df = me.ExperimentRegistry.from_cell_index(parquet, **cases.REGISTRY_KW)
    return {"registry": registry, "df": df, "golden": golden}


def dataset(world, device, budget=None, **kw):
    from viscy_amd.data import multi_experiment as me

    index = me.MultiExperimentIndex(registry=world["registry"], yx_patch_size=cases.YX_PATCH_SIZE, tau_range_hours=cases.TAU_RANGE_HOURS,
                                    cell_index_df=world["df"])
    return me.MultiExperimentTripletDataset(index=index, tau_range_hours=cases.TAU_RANGE_HOURS, device=device,
                                            device_cache_bytes=budget, **kw)


@pytest.mark.parametrize("mode", ["one_channel", "two_named"])
@pytest.mark.parametrize("budget", ["all", "one_frame", "zero"])
def test_device_batches_equal_host_path_batches(world, budget, mode):
    """mixed batches: both experiments (uint16 upsampled from 0.75, float32 downsampled from 1.5) in every batch"""
    kw = cases.DATASET_KW[mode]
    host = dataset(world, "cpu", **kw)
    dev = dataset(world, "cuda", {"all": 1 << 30, "one_frame": FRAME_BYTES["expA"], "zero": 0}[budget], **kw)
    assert host.cache is None and dev.cache.budget_bytes == {"all": 1 << 30, "one_frame": FRAME_BYTES["expA"], "zero": 0}[budget]
    order = np.random.default_rng(2).permutation(len(host)).tolist()
    C = 1 if mode == "one_channel" else 2
    for step in range(3):
        indices = order[8 * step : 8 * step + 8]
        assert len({host.index.valid_anchors["experiment"].iloc[i] for i in indices}) == 2
        host._rng, dev._rng = np.random.default_rng(step), np.random.default_rng(step)
        want, got = host.__getitems__(indices), dev.__getitems__(indices)
        assert sorted(got) == sorted(want) and got["anchor_meta"] == want["anchor_meta"] and got["positive_meta"] == want["positive_meta"]
        for key in ("anchor", "positive"):
            assert got[key].is_cuda and got[key].dtype == torch.float32 and tuple(got[key].shape) == (8, C, 6, *cases.YX_PATCH_SIZE)
            assert torch.equal(got[key].cpu().view(torch.int32), want[key].view(torch.int32)), (budget, step, key)
            for a, b in zip(got[f"{key}_norm_meta"], want[f"{key}_norm_meta"]):
                for ch in b:
                    for stat, value in b[ch]["timepoint_statistics"].items():
                        assert a[ch]["timepoint_statistics"][stat].is_cuda and a[ch]["timepoint_statistics"][stat].item() == value.item()
        assert dev.cache.bytes_used <= dev.cache.budget_bytes
    c = dev.cache
    if budget == "all":
        assert c.refused == 0 and c.evictions == 0 and c.uploads > 0 and c.hits > 0
    elif budget == "one_frame":   # an expA frame fits alone, an expB frame never does; a frame the batch needs is never evicted
        assert c.refused > 0 and c.uploads > 0 and len(c.keys()) == 1
        (resident,), evictions = c.keys(), c.evictions
        va = host.index.valid_anchors
        other = next(i for i in range(len(va)) if va["experiment"].iloc[i] == "expA"
                     and (va["fov_name"].iloc[i], int(va["t"].iloc[i])) != resident[1:])
        host._rng, dev._rng = np.random.default_rng(9), np.random.default_rng(9)
        want, got = host.__getitems__([other]), dev.__getitems__([other])
        assert c.evictions == evictions + 1 and len(c.keys()) == 1 and c.keys()[0][1:] == (va["fov_name"].iloc[other], int(va["t"].iloc[other]))
        for key in ("anchor", "positive"):   # the positive's frame (another time point) found the anchor's in its way: host-gathered
            assert torch.equal(got[key].cpu().view(torch.int32), want[key].view(torch.int32))
    else:
        assert c.uploads == 0 and c.refused > 0 and c.keys() == []


def test_golden_patches_on_the_device(world):
    """the reference's recorded patches straight from the device path"""
    for name in ("one_channel", "all_channels", "two_named"):
        ds, want = dataset(world, "cuda", **cases.DATASET_KW[name]), world["golden"]["dataset"][name]
        n = len(ds.index.valid_anchors)
        if ds._channel_mode == "from_index":
            forced = [[ds._va_arrays["channel_name"][i]] for i in range(n)]
        else:
            forced = None if ds._channel_mode == "all" else [ds._fixed_channel_names] * n
        for group, rec in want["patches"].items():
            boxes, _ = ds._slice_boxes(ds._va_arrays, rec["rows"], [forced[i] for i in rec["rows"]] if forced is not None else None)
            assert torch.equal(ds._cut(boxes).cpu().view(torch.int32), rec["patches"].view(torch.int32)), (name, group)


# ------------------------------------------------------------------------------------------------ a fit step
ENCODER = dict(backbone="convnext_tiny", in_channels=1, in_stack_depth=5, embedding_dim=64, projection_dim=32, depths=(1, 1, 2, 1),
               dims=(32, 64, 96, 128))   # the smallest configuration of tests/test_gpu_triplet.py
FIT_STORES = {
    "wide": dict(store="wide.zarr", dtype="uint16", T=3, Z=8, H=96, W=100, px=0.2, fovs=["A/1/0", "A/1/1"], interval=30.0),
    "fine": dict(store="fine.zarr", dtype="uint16", T=3, Z=12, H=160, W=150, px=0.1, fovs=["B/1/0", "B/1/1"], interval=30.0),
}
FIT_CHANNELS = ["Phase3D", "raw GFP EX488 EM525-45"]


@pytest.fixture(scope="module")
def fit_parquet(tmp_path_factory):
    """two experiments at 0.2 and 0.1 um per pixel (reference 0.15): native boxes of 48 and 96 pixels for 64-pixel patches"""
    import pandas as pd

    from viscy_amd.data import multi_experiment as me, write_hcs_plate

    root = tmp_path_factory.mktemp("multi_experiment_fit")
    rng = np.random.default_rng(5)
    rows = []
    for exp, s in FIT_STORES.items():
        arrays = {f: rng.integers(0, 4096, size=(s["T"], 2, s["Z"], s["H"], s["W"]), dtype=np.uint16) for f in s["fovs"]}
        write_hcs_plate(root / s["store"], arrays, FIT_CHANNELS)
        for fov in s["fovs"]:
            well, pos = fov.rsplit("/", 1)
            for track in range(4):
                y, x = int(rng.integers(s["H"] // 2 - 8, s["H"] // 2 + 8)), int(rng.integers(s["W"] // 2 - 8, s["W"] // 2 + 8))
                for t in range(s["T"]):
                    for ch in FIT_CHANNELS:
                        gtid = f"{exp}_{fov}_{track}"
                        rows.append(dict(
                            cell_id=f"{gtid}_{t}", experiment=exp, store_path=str(root / s["store"]), tracks_path="", fov=pos, well=well,
                            y=float(y), x=float(x), z=0, perturbation="mock" if track % 2 else "infected", channel_name=ch, t=t,
                            track_id=track, global_track_id=gtid, lineage_id=gtid, parent_track_id=-1,
                            hours_post_perturbation=t * 0.5, interval_minutes=s["interval"], microscope="", marker=ch.split()[-3] if " " in ch else ch,
                            organelle="", pixel_size_xy_um=s["px"], pixel_size_z_um=s["px"] * 2, T_shape=s["T"], C_shape=2,
                            Z_shape=s["Z"], Y_shape=s["H"], X_shape=s["W"], norm_mean=2048.0, norm_std=1182.0, norm_median=2048.0,
                            norm_iqr=2048.0))
    parquet = str(root / "cells.parquet")
    me.write_cell_index(pd.DataFrame(rows), parquet)
    return parquet


def test_a_fit_step_of_the_contrastive_module(fit_parquet):
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule
    from viscy_amd.data import MultiExperimentDataModule
    from viscy_amd.trainer import Trainer
    from viscy_amd.transforms import NormalizeSampled

    torch.manual_seed(0)
    enc = ContrastiveEncoder(**ENCODER)
    mod = ContrastiveModule(enc, lr=1e-3, example_input_array_shape=(1, 1, 5, 64, 64))
    enc.compute_dtype = torch.float32
    dm = MultiExperimentDataModule(
        fit_parquet, z_window=5, z_extraction_window=6, yx_patch_size=(72, 72), final_yx_patch_size=(64, 64), batch_size=4,
        split_ratio=0.5, tau_range=(0.5, 1.0), channels_per_sample=1, stratify_by="perturbation", seed=0,
        reference_pixel_size_xy_um=0.15, reference_pixel_size_z_um=0.3,
        normalizations=[NormalizeSampled(["channel_0"], level="timepoint_statistics")])
    tr = Trainer(max_epochs=1, precision="32-true", seed=0, limit_train_batches=1)
    tr.fit(mod, dm)
    assert tr.global_step == 1 and len(mod.logged["loss/train"]) == 1
    for key in ("loss/train", "loss/val"):
        assert mod.logged[key] and all(bool(torch.isfinite(v)) for v in mod.logged[key]), (key, mod.logged[key])
    cache = dm.train_dataset.cache
    assert cache.uploads > 0 and cache.refused == 0   # the batches came out of resident frames of both experiments
    sizes = {tuple(f.shape) for f in cache._frames.values()}
    assert sizes <= {(2, 8, 96, 100), (2, 12, 160, 150)}
