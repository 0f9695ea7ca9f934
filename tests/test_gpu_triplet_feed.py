"""GPU: the DynaCLR data feed end to end — a synthetic tracked plate written with this package's zarr writer, batches cut on
the device by vsx_patch_gather out of the frame cache, against the same batches cut on the host; then ContrastiveModule fed by
TripletDataModule through Trainer.fit / Trainer.predict and through the YAML entry point."""

import numpy as np
import pandas as pd
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
CHANNELS = ["Phase", "Nuclei"]
FOVS = ["A/1/0", "A/1/1", "B/1/0", "B/1/1"]
T, Z, H, W = 3, 5, 80, 72
PATCH = (64, 64)
ENCODER = dict(backbone="convnext_tiny", in_channels=1, in_stack_depth=5, embedding_dim=64, projection_dim=32, depths=(1, 1, 2, 1),
               dims=(32, 64, 96, 128))   # the smallest configuration of tests/test_gpu_triplet.py


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    from viscy_amd.data import write_hcs_plate

    root = tmp_path_factory.mktemp("feed")
    rng = np.random.default_rng(21)
    arrays = {name: rng.integers(0, 65536, size=(T, len(CHANNELS), Z, H, W), dtype=np.uint16) for name in FOVS}
    norm = {ch: {"fov_statistics": {"mean": 32768.0, "std": 18918.0}} for ch in CHANNELS}
    write_hcs_plate(root / "plate.zarr", arrays, CHANNELS, norm_meta=norm)
    for name in FOVS:
        rows = [{"track_id": k, "t": t, "id": k * T + t, "parent_track_id": -1, "parent_id": -1, "z": 2,
                 "y": int(rng.integers(33, H - 32)), "x": int(rng.integers(33, W - 32))} for k in range(6) for t in range(T)]
        (root / "tracks" / name).mkdir(parents=True)
        pd.DataFrame(rows).to_csv(root / "tracks" / name / "tracks.csv", index=False)
    return str(root / "plate.zarr"), str(root / "tracks"), arrays


def dataset(plate, device, budget=None):
    from viscy_amd.data import open_ome_zarr
    from viscy_amd.data.triplet import TripletDataset

    positions = [p for _, p in open_ome_zarr(plate[0]).positions()]
    tables = [pd.read_csv(f"{plate[1]}/{p.name}/tracks.csv").astype(int) for p in positions]
    return TripletDataset(positions, tables, ["Nuclei", "Phase"], PATCH, slice(1, 4), fit=True, time_interval=1, return_negative=True,
                          device=device, device_cache_bytes=budget)


FRAME_BYTES = 2 * 3 * H * W * 2   # two channels, three slices, uint16


@pytest.mark.parametrize("budget", ["all", "one_frame", "zero"])
def test_device_batches_equal_host_cut_batches(plate, budget):
    host = dataset(plate, "cpu")
    dev = dataset(plate, "cuda", {"all": None, "one_frame": FRAME_BYTES, "zero": 0}[budget])
    assert host.cache is None and dev.cache.budget_bytes == {"all": len(FOVS) * T * FRAME_BYTES, "one_frame": FRAME_BYTES, "zero": 0}[budget]
    order = np.random.default_rng(2).permutation(len(host)).tolist()
    for step in range(3):
        indices = order[8 * step : 8 * step + 8]
        np.random.seed(step)
        want = host.__getitems__(indices)
        np.random.seed(step)
        got = dev.__getitems__(indices)
        assert sorted(got) == sorted(want)
        for key in ("anchor", "positive", "negative"):
            assert got[key].is_cuda and got[key].dtype == torch.float32 and tuple(got[key].shape) == (8, 2, 3, 64, 64)
            assert torch.equal(got[key].cpu().view(torch.int32), want[key].view(torch.int32)), (budget, step, key)
        # the plate's own values, channel order as asked (Nuclei first)
        row = host.valid_anchors.iloc[indices[0]]
        y, x = int(row["y"]), int(row["x"])
        ref = plate[2][row["fov_name"]][int(row["t"]), [1, 0], 1:4, y - 32 : y + 32, x - 32 : x + 32].astype(np.float32)
        assert torch.equal(got["anchor"][0].cpu(), torch.from_numpy(ref))
        assert dev.cache.bytes_used <= dev.cache.budget_bytes
    c = dev.cache
    if budget == "all":
        assert c.refused == 0 and c.evictions == 0 and 0 < c.uploads <= len(FOVS) * T and c.hits > 0
    elif budget == "one_frame":
        assert c.refused > 0 and c.uploads > 0 and len(c.keys()) == 1   # one frame resident, the others cut on the host
    else:
        assert c.uploads == 0 and c.refused > 0 and c.keys() == []


def _module(loss=None):
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule

    torch.manual_seed(0)
    enc = ContrastiveEncoder(**ENCODER)
    mod = ContrastiveModule(enc, loss_function=loss, lr=1e-3, example_input_array_shape=(1, 1, 5, 64, 64))
    enc.compute_dtype = torch.float32
    return mod


def _datamodule(plate, **kw):
    from viscy_amd.data.triplet import TripletDataModule
    from viscy_amd.transforms import NormalizeSampled

    return TripletDataModule(plate[0], plate[1], source_channel=["Phase"], z_range=(0, 5), initial_yx_patch_size=PATCH,
                             final_yx_patch_size=PATCH, batch_size=4, split_ratio=0.75,
                             normalizations=[NormalizeSampled(["Phase"], level="fov_statistics")], **kw)


@pytest.mark.parametrize("loss", ["ntxent", "triplet"])
def test_two_fit_steps_of_the_contrastive_module(plate, loss):
    from viscy_amd.trainer import Trainer

    if loss == "ntxent":
        mod, dm = _module(), _datamodule(plate, time_interval="any", return_negative=False)
    else:
        mod, dm = _module(nn.TripletMarginLoss(margin=0.5)), _datamodule(plate, time_interval=1, return_negative=True)
    np.random.seed(0)
    tr = Trainer(max_epochs=1, precision="32-true", seed=0, limit_train_batches=2)
    tr.fit(mod, dm)
    assert tr.global_step == 2 and len(mod.logged["loss/train"]) == 2
    for key in ("loss/train", "loss/val"):
        assert all(bool(torch.isfinite(v)) for v in mod.logged[key]), (key, mod.logged[key])
    assert len(mod.logged["loss/val"]) == -(-len(dm.val_dataset) // 4)
    assert dm.train_dataset.cache.uploads > 0 and dm.train_dataset.cache.refused == 0   # the batches came out of resident frames


def test_predict_pass_follows_the_track_table(plate):
    from viscy_amd.trainer import Trainer

    mod, dm = _module(), _datamodule(plate)
    tr = Trainer(precision="32-true")
    outs = tr.predict(mod, dm)
    assert not tr.predicting
    tracks = dm.predict_dataset.tracks
    assert len(tracks) == len(FOVS) * 6 * T and len(outs) == -(-len(tracks) // 4)
    index = [d for o in outs for d in o["index"]]
    assert [(d["fov_name"], int(d["track_id"]), int(d["t"])) for d in index] == \
        list(zip(tracks["fov_name"], (int(v) for v in tracks["track_id"]), (int(v) for v in tracks["t"])))
    assert list(index[0]) == ["fov_name", "track_id", "t", "id", "parent_track_id", "parent_id", "z", "y", "x"]
    for key in ("features", "projections"):
        rows = torch.cat([o[key] for o in outs])
        assert rows.ndim == 2 and rows.shape[0] == len(tracks) and bool(torch.isfinite(rows).all()), key
    assert rows.shape[1] == ENCODER["projection_dim"]
    c = dm.predict_dataset.cache
    assert c.uploads == len(FOVS) * T and c.refused == 0   # table order: every frame uploaded once, serving all of its cells


def test_yaml_recipe_runs_fit_and_predict(plate, tmp_path):
    import yaml

    from viscy_amd import config

    recipe = {
        "seed_everything": 0,
        "trainer": {"fast_dev_run": True, "precision": "32-true"},
        "model": {"class_path": "dynaclr.engine.ContrastiveModule", "init_args": {
            "encoder": {"class_path": "viscy_models.contrastive.ContrastiveEncoder",
                        "init_args": {k: list(v) if isinstance(v, tuple) else v for k, v in ENCODER.items()}},
            "example_input_array_shape": [1, 1, 5, 64, 64]}},
        "data": {"class_path": "viscy_data.triplet.TripletDataModule", "init_args": {
            "data_path": plate[0], "tracks_path": plate[1], "source_channel": ["Phase"], "z_range": [0, 5],
            "initial_yx_patch_size": [64, 64], "final_yx_patch_size": [64, 64], "batch_size": 4, "return_negative": False,
            "normalizations": [{"class_path": "viscy_transforms.NormalizeSampled",
                                "init_args": {"keys": ["Phase"], "level": "fov_statistics"}}]}},
    }
    path = tmp_path / "recipe.yml"
    path.write_text(yaml.safe_dump(recipe))
    assert config.main(["fit", "--config", str(path)]) == 0
    recipe["data"]["init_args"].update(predict_cells=True, include_fov_names=["A/1/1"], include_track_ids=[3])
    path.write_text(yaml.safe_dump(recipe))
    assert config.main(["predict", "--config", str(path)]) == 0
