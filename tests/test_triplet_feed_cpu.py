"""CPU: viscy_amd.data.triplet (TripletDataset / TripletDataModule / FrameCache) and the host side of ops.patch_gather.

tests/golden/triplet.pt holds what the reference's TripletDataset made of a small tracked plate (tools/make_triplet_golden.py):
the tables it filtered, the rows it drew under np.random.seed, the patches it cut and its predict-mode index dicts.  The plate is
rebuilt here from the fixture's arrays with this package's zarr writer; without a HIP device the dataset cuts on the host."""

import functools

import numpy as np
import pandas as pd
import pytest
import torch

from tests.conftest import load_golden

FIT_CASES = ["any_neg", "any_noneg", "t1_neg", "t1_noneg"]


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("triplet.pt")


def write_plate(root, images=None, dtype=None, drop_columns=(), fovs=None):
    """the fixture's plate as an OME-Zarr store plus tracks/<fov>/tracks.csv; -> (data_path, tracks_path)"""
    from viscy_amd.data import write_hcs_plate

    g = golden()
    fovs = fovs or g["fovs"]
    arrays = {k: (images[k] if images else g["images"][k].numpy()) for k in fovs}
    if dtype is not None:
        arrays = {k: v.astype(dtype) for k, v in arrays.items()}
    write_hcs_plate(root / "plate.zarr", arrays, g["channels"], norm_meta=g["norm_meta"])
    for k in fovs:
        d = root / "tracks" / k
        d.mkdir(parents=True, exist_ok=True)
        pd.DataFrame(g["tracks_tables"][k]).drop(columns=list(drop_columns)).to_csv(d / "tracks.csv", index=False)
    return root / "plate.zarr", root / "tracks"


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    return write_plate(tmp_path_factory.mktemp("triplet"))


def make_dataset(plate, device="cpu", **kw):
    from viscy_amd.data import open_ome_zarr
    from viscy_amd.data.triplet import TripletDataset

    g = golden()
    data_path, tracks_path = plate
    positions = [p for _, p in open_ome_zarr(data_path).positions()]
    assert [p.name for p in positions] == g["fovs"]
    tables = [pd.read_csv(next((tracks_path / p.name).glob("*.csv"))).astype(int) for p in positions]
    kw.setdefault("z_range", slice(*g["z_range"]))
    kw.setdefault("initial_yx_patch_size", g["initial_yx_patch_size"])
    return TripletDataset(positions, tables, g["source_channel"], device=device, **kw)


def as_table(df):
    return {"index": [int(i) for i in df.index], "columns": {c: [v if isinstance(v, str) else int(v) for v in df[c]] for c in df.columns}}


@pytest.mark.parametrize("tag", FIT_CASES)
def test_tables_and_draws_equal_the_reference(plate, tag):
    case = golden()["cases"][tag]
    ds = make_dataset(plate, fit=True, **case["kwargs"])
    assert len(ds) == case["len"]
    assert as_table(ds.tracks) == case["tracks"]
    assert as_table(ds.valid_anchors) == case["valid_anchors"]
    assert len(ds.tracks) < sum(len(t["t"]) for t in golden()["tracks_tables"].values())   # the border filter removed rows
    anchor_rows = ds.valid_anchors.iloc[case["indices"]]
    assert as_table(anchor_rows) == case["anchor_rows"]
    if "positive_rows" in case:
        assert as_table(ds._sample_positives(anchor_rows)) == case["positive_rows"]
    if "negative_rows" in case:
        np.random.seed(case["seed"])
        assert as_table(ds._sample_negatives(anchor_rows)) == case["negative_rows"]


@pytest.mark.parametrize("tag", FIT_CASES)
def test_host_cut_batches_equal_the_reference(plate, tag):
    case = golden()["cases"][tag]
    ds = make_dataset(plate, fit=True, **case["kwargs"])
    np.random.seed(case["seed"])
    sample = ds.__getitems__(case["indices"])
    keys = [k for k in ("anchor", "positive", "negative") if k in case]
    assert sorted(sample) == sorted(keys + [f"{k}_norm_meta" for k in keys])
    for k in keys:
        assert sample[k].dtype == torch.float32 and sample[k].device.type == "cpu"
        assert tuple(sample[k].shape) == (len(case["indices"]), 2, 2, 12, 10)   # (13, 10) asked: 2 * (13 // 2) rows
        assert torch.equal(sample[k], case[k].to(torch.float32)), k
        assert len(sample[f"{k}_norm_meta"]) == len(case["indices"])
    got = [float(m["Phase"]["fov_statistics"]["mean"]) for m in sample["anchor_norm_meta"]]
    assert got == case["anchor_norm_mean_Phase"]
    if case["kwargs"]["time_interval"] == "any":
        assert torch.equal(sample["positive"], sample["anchor"])


@pytest.mark.parametrize("tag", ["predict", "predict_cells"])
def test_predict_index_and_patches_equal_the_reference(plate, tag):
    case = golden()["cases"][tag]
    ds = make_dataset(plate, fit=False, **case["kwargs"])
    assert len(ds) == case["len"] and as_table(ds.tracks) == case["tracks"]
    sample = ds.__getitems__(case["indices"])
    assert sorted(sample) == ["anchor", "anchor_norm_meta", "index"]
    assert torch.equal(sample["anchor"], case["anchor"].to(torch.float32))
    index = [{k: (v if isinstance(v, str) else int(v)) for k, v in d.items()} for d in sample["index"]]
    assert index == case["index"]
    assert list(index[0]) == golden()["index_columns"]


def test_channel_order_and_extent_against_the_array(plate):
    """the patch is the requested channels in the requested order, the Z range, and slice(c - s // 2, c + s // 2) in y and x"""
    from viscy_amd.data.triplet import patch_extent

    assert patch_extent(20, 13) == (14, 12) and patch_extent(20, 10) == (15, 10) and patch_extent(7, 1) == (7, 0)
    g = golden()
    ds = make_dataset(plate, fit=False)
    row = ds.valid_anchors.iloc[5]
    img = g["images"][row["fov_name"]].numpy()
    ch = [g["channels"].index(c) for c in g["source_channel"]]
    assert ch == [1, 0]
    y, x = int(row["y"]), int(row["x"])
    want = img[int(row["t"])][ch][:, g["z_range"][0]:g["z_range"][1], y - 6 : y + 6, x - 5 : x + 5].astype(np.float32)
    assert torch.equal(ds.__getitems__([5])["anchor"][0], torch.from_numpy(want))


def test_exceptions(tmp_path, plate):
    from viscy_amd.data.triplet import TripletDataModule, host_cut

    with pytest.raises(ValueError, match=r"Z range slice\(1, 4, None\) exceeds image with Z=3"):
        make_dataset(plate, z_range=slice(1, 4))
    no_z = write_plate(tmp_path / "no_z", drop_columns=("z",), fovs=["A/1/0"])
    g = golden()
    kw = dict(source_channel=g["source_channel"], z_range=g["z_range"], initial_yx_patch_size=g["initial_yx_patch_size"],
              final_yx_patch_size=(12, 10), batch_size=4)
    dm = TripletDataModule(*map(str, no_z), **kw)
    dm.device = "cpu"
    dm.setup("predict")
    batch = next(iter(dm.predict_dataloader()))
    assert "z" not in batch["index"][0] and list(batch["index"][0]) == [c for c in g["index_columns"] if c != "z"]
    no_parent = write_plate(tmp_path / "no_parent", drop_columns=("parent_id",), fovs=["A/1/0"])
    dm = TripletDataModule(*map(str, no_parent), **kw)
    dm.device = "cpu"
    dm.setup("predict")
    with pytest.raises(KeyError, match="Required column 'parent_id' not found in data"):
        next(iter(dm.predict_dataloader()))
    with pytest.raises(NotImplementedError, match="Self-supervised model does not support testing"):
        dm.setup("test")
    with pytest.raises(NotImplementedError, match="other stage"):
        dm.setup("other")
    f64 = write_plate(tmp_path / "f64", dtype=np.float64, fovs=["A/1/0"])
    dm = TripletDataModule(*map(str, f64), **kw)
    with pytest.raises(NotImplementedError, match="float64"):
        dm.setup("predict")
    frame = np.zeros((1, 1, 8, 9), np.uint8)
    for y0, x0 in ((-1, 0), (5, 0), (0, -1), (0, 4)):
        with pytest.raises(ValueError, match="leave the frame"):
            host_cut(frame, y0, x0, 4, 6)
    assert host_cut(frame, 4, 3, 4, 6).shape == (1, 1, 4, 6)
    with pytest.warns(UserWarning, match="more than 1 thread worker"):
        TripletDataModule(*map(str, plate), num_workers=2, **kw)


class _Trainer:
    def __init__(self, predicting=False):
        self.predicting = predicting


def test_find_transform_table(plate):
    from viscy_amd.data.triplet import TripletDataModule

    g = golden()

    def module(**kw):
        return TripletDataModule(*map(str, plate), source_channel=g["source_channel"], z_range=g["z_range"], **kw)

    for interval, anchor_augmented in (("any", False), (0, False), (1, True)):
        dm = module(time_interval=interval)
        aug, plain = dm._augmentation_transform, dm._no_augmentation_transform
        assert aug is not plain
        # no trainer attached: the key rule alone
        assert dm._find_transform("anchor") is (aug if anchor_augmented else plain)
        assert dm._find_transform("positive") is aug and dm._find_transform("negative") is aug
        dm.trainer = _Trainer()
        dm.training = True
        assert dm._find_transform("anchor") is (aug if anchor_augmented else plain) and dm._find_transform("positive") is aug
        dm.training = False   # validating, augment_validation=True (the default): as in training
        assert dm._find_transform("anchor") is (aug if anchor_augmented else plain) and dm._find_transform("positive") is aug
        dm.trainer = _Trainer(predicting=True)
        for key in ("anchor", "positive", "negative"):
            assert dm._find_transform(key) is plain
    dm = module(time_interval=1, augment_validation=False)
    dm.trainer = _Trainer()
    dm.training = False
    for key in ("anchor", "positive", "negative"):
        assert dm._find_transform(key) is dm._no_augmentation_transform
    dm.training = True
    assert dm._find_transform("anchor") is dm._augmentation_transform


class _Record:
    """a dict transform that writes down what it is handed and scales each channel by its own factor"""

    def __init__(self, log, factors):
        self.log, self.factors = log, factors

    def __call__(self, sample):
        self.log.append({k: (tuple(v.shape) if torch.is_tensor(v) else v) for k, v in sample.items()})
        out = {k: (v * self.factors[k] if k in self.factors else v) for k, v in sample.items()}
        return out


def test_channel_wise_transform_order_and_shape_check(plate):
    from viscy_amd.data.triplet import TripletDataModule
    from viscy_amd.transforms import NormalizeSampled

    g = golden()
    log = []
    dm = TripletDataModule(*map(str, plate), source_channel=g["source_channel"], z_range=g["z_range"], initial_yx_patch_size=(13, 10),
                           final_yx_patch_size=(12, 10), batch_size=3, time_interval=1, return_negative=True, split_ratio=0.5,
                           normalizations=[NormalizeSampled(["Phase"], level="fov_statistics")],
                           augmentations=[_Record(log, {"Nuclei": 2.0, "Phase": -1.0})])
    dm.device = "cpu"
    torch.manual_seed(0)
    dm.setup("fit")
    np.random.seed(0)
    raw = dm.train_dataset.__getitems__([0, 1, 2])
    np.random.seed(0)
    batch = dm.on_after_batch_transfer(dm.train_dataset.__getitems__([0, 1, 2]), 0)
    assert sorted(batch) == ["anchor", "negative", "positive"]   # the *_norm_meta lists are consumed
    # three keys went through the augmenting chain: channels under their names in source_channel order, (B, 1, Z, Y, X) each,
    # with the collated (B,) statistics
    assert len(log) == 3
    for entry in log:
        assert list(entry)[:2] == ["Nuclei", "Phase"] and entry["Nuclei"] == entry["Phase"] == (3, 1, 2, 12, 10)
        assert tuple(entry["norm_meta"]["Phase"]["fov_statistics"]["mean"].shape) == (3,)
    mean, std = g["norm_meta"]["Phase"]["fov_statistics"]["mean"], g["norm_meta"]["Phase"]["fov_statistics"]["std"]
    for key in ("anchor", "positive", "negative"):
        want = torch.cat((raw[key][:, 0:1] * 2.0, -((raw[key][:, 1:2] - mean) / (std + 1e-8))), dim=1)
        torch.testing.assert_close(batch[key], want, rtol=1e-6, atol=1e-6)
    dm.yx_patch_size = (12, 12)
    np.random.seed(0)
    with pytest.raises(ValueError, match=r"Spatial shape mismatch for 'anchor': got \(2, 12, 10\), expected \(2, 12, 12\)"):
        dm.on_after_batch_transfer(dm.train_dataset.__getitems__([0]), 0)
    t = torch.zeros(2, 3)
    assert dm.on_after_batch_transfer(t, 0) is t


def test_setup_split_filters_and_loaders(plate):
    from viscy_amd.data.triplet import TripletDataModule

    g = golden()
    kw = dict(source_channel=g["source_channel"], z_range=g["z_range"], initial_yx_patch_size=g["initial_yx_patch_size"],
              final_yx_patch_size=(12, 10), batch_size=4)
    dm = TripletDataModule(*map(str, plate), split_ratio=0.5, **kw)
    dm.device = "cpu"
    torch.manual_seed(3)
    dm.setup("fit")
    torch.manual_seed(3)
    order = torch.randperm(4).tolist()   # the global torch state, then int(n * split_ratio)
    names = [g["fovs"][i] for i in order]
    assert [p.name for p in dm.train_dataset.positions] == names[:2] and [p.name for p in dm.val_dataset.positions] == names[2:]
    assert dm.z_window_size == 2 and dm.yx_patch_size == (12, 10)
    train = dm.train_dataloader()
    assert len(train) == len(dm.train_dataset) // 4   # drop_last
    assert isinstance(train.sampler, torch.utils.data.RandomSampler) and train.num_workers == 0
    val = dm.val_dataloader()
    assert isinstance(val.sampler, torch.utils.data.SequentialSampler) and len(val) == -(-len(dm.val_dataset) // 4)
    np.random.seed(0)
    batch = next(iter(train))
    assert tuple(batch["anchor"].shape) == (4, 2, 2, 12, 10) and len(batch["negative_norm_meta"]) == 4
    # well / FOV filters
    dm = TripletDataModule(*map(str, plate), fit_include_wells=["B/2"], fit_exclude_fovs=["A/1/0"], split_ratio=0.5, **kw)
    dm.device = "cpu"
    dm.setup("fit")
    assert sorted(p.name for p in dm.train_dataset.positions + dm.val_dataset.positions) == ["B/2/0", "B/2/1"]
    assert len(dm.train_dataset.positions) == 1 and set(dm.train_dataset.tracks["fov_name"]) == {dm.train_dataset.positions[0].name}
    dm = TripletDataModule(*map(str, plate), fit_exclude_fovs=["A/1/1", "B/2/1"], split_ratio=0.5, **kw)
    dm.device = "cpu"
    dm.setup("fit")
    assert sorted(p.name for p in dm.train_dataset.positions + dm.val_dataset.positions) == ["A/1/0", "B/2/0"]
    # predict visits the cells in track-table order
    dm = TripletDataModule(*map(str, plate), **kw)
    dm.device = "cpu"
    dm.setup("predict")
    seen = [(d["fov_name"], int(d["id"])) for b in dm.predict_dataloader() for d in b["index"]]
    tracks = dm.predict_dataset.tracks
    assert seen == list(zip(tracks["fov_name"], (int(v) for v in tracks["id"]))) and len(seen) == golden()["cases"]["predict"]["len"]


# ------------------------------------------------------------------------------------------------ FrameCache
def _cache(budget, sizes=None):
    from viscy_amd.data.triplet import FrameCache

    loads = []

    def load(key):
        loads.append(key)
        return np.full((1, 1, 2, (sizes or {}).get(key, 50)), hash(key) % 251, np.uint8)

    def nbytes(key):
        return 2 * (sizes or {}).get(key, 50)

    return FrameCache(load, nbytes, "cpu", budget), loads


def test_frame_cache_budget_lru_and_current_batch():
    cache, loads = _cache(300)   # three frames of 100 bytes
    a, b, c, d, e = (("f", t) for t in range(5))
    got = cache.begin_batch([a, b, a, c])
    assert list(got) == [a, b, c] and all(v is not None for v in got.values()) and loads == [a, b, c]
    assert cache.keys() == [a, b, c] and cache.bytes_used == 300 and got[a].dtype == torch.uint8 and tuple(got[a].shape) == (1, 1, 2, 50)
    cache.begin_batch([a])                       # a hit refreshes: b is now the least recently used
    assert cache.keys() == [b, c, a] and cache.hits == 1 and loads == [a, b, c]
    got = cache.begin_batch([d])                 # evicts b only
    assert cache.keys() == [c, a, d] and cache.evictions == 1 and got[d] is not None and cache.bytes_used == 300
    # the batch needs c and a (resident) and two more: one fits after evicting d, the other finds nothing left to evict
    got = cache.begin_batch([c, b, a, e])
    assert got[c] is not None and got[a] is not None and got[b] is not None and got[e] is None
    assert cache.keys() == [c, b, a] and cache.refused == 1 and cache.bytes_used == 300 and e not in cache
    # a frame needed by the current batch is never evicted, in whatever order the keys come
    got = cache.begin_batch([e, c, b, a])
    assert got[e] is None and all(got[k] is not None for k in (a, b, c)) and cache.keys() == [c, b, a]
    assert cache.bytes_used <= cache.budget_bytes


def test_frame_cache_too_small_falls_back_and_sizes_differ():
    cache, loads = _cache(0)
    got = cache.begin_batch([("f", 0), ("f", 1)])
    assert got == {("f", 0): None, ("f", 1): None} and loads == [] and cache.bytes_used == 0 and cache.refused == 2
    sizes = {"big": 200, "s1": 40, "s2": 40, "s3": 40}
    cache, loads = _cache(250, sizes)            # bytes: big 400, small 80
    assert cache.begin_batch(["big"])["big"] is None and loads == []     # larger than the whole budget: nothing is evicted for it
    cache.begin_batch(["s1", "s2", "s3"])
    assert cache.bytes_used == 240 and cache.keys() == ["s1", "s2", "s3"]
    cache, _ = _cache(450, sizes)
    cache.begin_batch(["s1", "s2"])
    cache.begin_batch(["big"])                   # 160 + 400 > 450: both small frames go, least recently used first
    assert cache.keys() == ["big"] and cache.bytes_used == 400 and cache.evictions == 2
    cache.begin_batch(["s3"])                    # 480 > 450: big goes
    assert cache.keys() == ["s3"] and cache.bytes_used == 80


# ------------------------------------------------------------------------------------------------ ops.patch_gather, host side
def test_descriptor_validation_and_contents():
    from viscy_amd import _lib, ops

    block = torch.zeros(2, 3, 4, 20, 37, dtype=torch.uint16)
    frame = block[1, :, 1:3, 2:18, 5:35]         # (3, 2, 16, 30): a view into the larger block
    size = (4, 6)
    table = ops.patch_descriptors([frame, frame, block[0, :, :2]], [(0, 0), (12, 24), (16, 31)], size)
    assert table.dtype == torch.int64 and tuple(table.shape) == (3, _lib.PG_DESC)
    assert table[0].tolist() == [frame.data_ptr(), 4 * 20 * 37, 20 * 37, 37, 0, 0]
    assert table[1].tolist() == [frame.data_ptr(), 4 * 20 * 37, 20 * 37, 37, 12, 24]   # flush with the view's last row and column
    assert table[2].tolist() == [block.data_ptr(), 4 * 20 * 37, 20 * 37, 37, 16, 31]
    for origin in ((-1, 0), (13, 0), (0, -1), (0, 25)):
        with pytest.raises(ValueError, match="leave the frame"):
            ops.patch_descriptors([frame], [origin], size)
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.patch_descriptors([frame.transpose(2, 3)], [(0, 0)], size)
    with pytest.raises(ValueError, match="one launch serves"):
        ops.patch_descriptors([frame, block[0, :2, :2]], [(0, 0), (0, 0)], size)
    with pytest.raises(ValueError, match="1 frames for 2 origins"):
        ops.patch_descriptors([frame], [(0, 0), (0, 0)], size)
    for dt in (torch.float64, torch.int32, torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match=str(dt)):
            ops.patch_descriptors([torch.zeros(1, 1, 8, 8, dtype=dt)], [(0, 0)], size)
    for dt in (torch.float32, torch.uint16, torch.int16, torch.uint8):
        ops.patch_descriptors([torch.zeros(1, 1, 8, 8, dtype=dt)], [(4, 2)], size)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.patch_gather([frame], [(0, 0)], size)
    assert "vsx_patch_gather" in _lib.exported_symbols()


def test_yaml_class_map_resolves_both_paths(plate):
    from viscy_amd import config
    from viscy_amd.data.triplet import TripletDataModule

    g = golden()
    for path in ("viscy_data.triplet.TripletDataModule", "viscy_data.TripletDataModule"):
        assert config._resolve(path) is TripletDataModule
        dm = config.instantiate({"class_path": path, "init_args": {
            "data_path": str(plate[0]), "tracks_path": str(plate[1]), "source_channel": g["source_channel"], "z_range": [1, 3],
            "initial_yx_patch_size": [13, 10], "final_yx_patch_size": [12, 10], "batch_size": 2, "device_cache_bytes": 1 << 20,
            "normalizations": [{"class_path": "viscy_transforms.NormalizeSampled",
                                "init_args": {"keys": ["Phase"], "level": "fov_statistics"}}]}})
        assert isinstance(dm, TripletDataModule) and dm.device_cache_bytes == 1 << 20 and dm.z_range == slice(1, 3)
