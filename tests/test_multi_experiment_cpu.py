"""CPU: the multi-experiment DynaCLR feed (viscy_amd/data/multi_experiment.py) against what the reference's own classes computed
on the synthetic two-experiment data set (tests/golden/multi_experiment.pt, tools/gen_golden_multi_experiment.py,
tests/multi_experiment_cases.py): the sampler batch for batch, tau draws, the index's anchors and clamped centres, the native
boxes, target sizes and resampled patches of the host path (bit-equal), norm-meta trees, label ids, predict index dicts; the
resampling map against CPU torch over the full range; positives by property; the data module's transform round."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import multi_experiment_cases as cases
from tests.conftest import load_golden
from viscy_amd.data import multi_experiment as me


@pytest.fixture(scope="module")
def golden():
    return load_golden("multi_experiment.pt")


@pytest.fixture(scope="module")
def world(golden, tmp_path_factory):
    """the two plates and the parquet on disk, the registry and the table read back from it"""
    root = tmp_path_factory.mktemp("multi_experiment")
    cases.write_stores(root)
    parquet = str(root / "cells.parquet")
    me.write_cell_index(cases.table_frame(golden["table"], root), parquet)
    registry, df = me.ExperimentRegistry.from_cell_index(parquet, **cases.REGISTRY_KW)
    return {"root": root, "parquet": parquet, "registry": registry, "df": df}


def make_index(world, **kw):
    return me.MultiExperimentIndex(registry=world["registry"], yx_patch_size=cases.YX_PATCH_SIZE, tau_range_hours=cases.TAU_RANGE_HOURS,
                                   cell_index_df=world["df"], **kw)


def make_dataset(world, index_kw=None, fit=True, **kw):
    index = make_index(world, **(index_kw if index_kw is not None else cases.INDEX_KW["temporal_default_shift"]))
    return me.MultiExperimentTripletDataset(index=index, fit=fit, tau_range_hours=cases.TAU_RANGE_HOURS, device="cpu", **kw)


def row_ids(df):
    return [f"{c}|{ch}" for c, ch in zip(df["cell_id"].astype(str), df["channel_name"].astype(str))]


def plain(v):
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if torch.is_tensor(v):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, np.ndarray):
        return v.tolist()
    return v


# ------------------------------------------------------------------------------------------------ the resampling map
def test_nearest_exact_index_is_torchs_map_on_every_axis_of_a_5d_tensor():
    """all 1 <= in, out <= 96, along Z, Y and X of a 5-D arange (the call ``_rescale_patch`` makes)"""
    sizes, base = range(1, 97), [2, 3, 3]
    for i in sizes:
        src = torch.arange(i, dtype=torch.float32)
        vols = []
        for axis in range(3):
            shape, view = list(base), [1, 1, 1, 1, 1]
            shape[axis], view[2 + axis] = i, i
            vols.append(src.reshape(view).expand(1, 1, *shape).contiguous())
        for o in sizes:
            want = me.nearest_exact_index(i, o)
            assert want.dtype == np.int64 and want.shape == (o,)
            for axis, vol in enumerate(vols):
                size = list(base)
                size[axis] = o
                line = F.interpolate(vol, size=tuple(size), mode="nearest-exact").movedim(2 + axis, -1).reshape(-1, o)
                assert bool((line == line[0]).all())
                assert np.array_equal(line[0].to(torch.int64).numpy(), want), (i, o, axis)
    assert me.nearest_exact_index(7, 5) is me.nearest_exact_index(7, 5) and not me.nearest_exact_index(7, 5).flags.writeable
    with pytest.raises(ValueError):
        me.nearest_exact_index(0, 4)


def test_host_gather_checks_every_axis():
    frame = np.arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5)
    got = me.host_gather(frame, [1, 0], [2, 2], [0, 3], [4, 0, 4])
    assert got.shape == (2, 2, 2, 3) and got[0, 0, 1, 0] == frame[1, 2, 3, 4]
    for axis, name in enumerate(("channel", "z", "y", "x")):
        tabs = [[0], [0], [0], [0]]
        tabs[axis] = [frame.shape[axis]]
        with pytest.raises(ValueError, match=f"{name} table"):
            me.host_gather(frame, *tabs)


def test_patch_tables_tells_temporary_table_objects_apart():
    """tables handed over as rows of a 2-D int32 array, tensor rows or fresh lists are temporaries: each ``ys[i]`` is a new object
    that may take the address of the one before.  Every patch keeps its own table, every table is checked, and an object
    that really is shared is stored once."""
    from viscy_amd import ops

    frame = torch.zeros(2, 3, 16, 16)
    n = 4
    chans, zs, xs = [np.arange(2)] * n, [np.arange(3)] * n, [np.arange(8)] * n
    rows = np.stack([i + np.arange(8) for i in range(n)]).astype(np.int32)
    for ys in (rows, torch.from_numpy(rows), [[int(v) for v in r] for r in rows], [tuple(int(v) for v in r) for r in rows]):
        desc, idx, shape = ops.patch_tables([frame] * n, chans, zs, ys, xs)
        assert shape == (n, 2, 3, 8, 8)
        for i in range(n):
            off = int(desc[i, 6])
            assert idx[off : off + 8].tolist() == rows[i].tolist(), i
        assert len({int(v) for v in desc[:, 6]}) == n and len({int(v) for v in desc[:, 7]}) == 1   # four y tables, one shared x table
    frames5 = torch.zeros(n, 2, 3, 16, 16)   # frames[i] of a 5-D tensor are temporaries too
    desc, _, _ = ops.patch_tables(frames5, chans, zs, rows, xs)
    assert [int(v) for v in desc[:, 0]] == [frames5[i].data_ptr() for i in range(n)]
    bad = rows.copy()
    bad[3, -1] = 16   # only the LAST patch's table leaves the frame: it must be the one that is checked and named
    with pytest.raises(ValueError, match="patch 3 y table"):
        ops.patch_tables([frame] * n, chans, zs, bad, xs)


# ------------------------------------------------------------------------------------------------ sampler, tau
@pytest.mark.parametrize("name", list(cases.SAMPLER_KW))
def test_sampler_is_the_references_batch_for_batch(golden, world, name):
    anchors = make_index(world, **cases.INDEX_KW["temporal_default_shift"]).valid_anchors
    kw = cases.SAMPLER_KW[name]
    for seed in cases.SAMPLER_SEEDS:
        for rank, want in enumerate(golden["sampler"][name][seed]):
            s = me.FlexibleBatchSampler(anchors, seed=seed, rank=rank, **kw)
            assert len(s) == want["length"] == math.ceil((len(anchors) // kw["batch_size"]) / kw.get("num_replicas", 1))
            assert [list(s) for _ in range(cases.SAMPLER_EPOCHS)] == want["epochs"]
            assert want["epochs"][0] != want["epochs"][1]
            s.set_epoch(5)
            assert list(s) == want["after_set_epoch_5"]


def test_sampler_refuses_missing_columns(world):
    anchors = make_index(world, **cases.INDEX_KW["self"]).valid_anchors
    with pytest.raises(ValueError, match="stratify_by"):
        me.FlexibleBatchSampler(anchors, stratify_by="nope")
    with pytest.raises(ValueError, match="batch_group_by"):
        me.FlexibleBatchSampler(anchors, batch_group_by="nope", stratify_by=None)
    with pytest.raises(ValueError, match="hours_post_perturbation"):
        me.FlexibleBatchSampler(anchors.drop(columns=["hours_post_perturbation"]), stratify_by=None, temporal_enrichment=True)


def test_sample_tau_and_temporal_candidates_with_an_injected_generator(golden):
    for rec in golden["sample_tau"]:
        tau_min, tau_max, decay = rec["args"]
        rng = np.random.default_rng(rec["seed"])
        assert [me.sample_tau(tau_min, tau_max, rng, decay) for _ in rec["draws"]] == rec["draws"]
    timepoints, markers = golden["pick_temporal"]["timepoints"], np.array(golden["pick_temporal"]["markers"], dtype=object)
    for rec in golden["pick_temporal"]["cases"]:
        anchor_t, tau_min, tau_max, use_markers, anchor_marker = rec["args"]
        rng = np.random.default_rng(rec["seed"])
        got = [me._pick_temporal_candidate(timepoints, anchor_t, tau_min, tau_max, 2.0, rng, markers if use_markers else None,
                                           anchor_marker) for _ in rec["picks"]]
        assert got == rec["picks"]


# ------------------------------------------------------------------------------------------------ registry, index
def test_registry_from_the_parquet(golden, world):
    r, want = world["registry"], golden["registry"]
    assert plain(r.z_ranges) == want["z_ranges"] and plain(r.scale_factors) == want["scale_factors"]
    assert {e.name: list(r.tau_range_frames(e.name, cases.TAU_RANGE_HOURS)) for e in r.experiments} == want["tau_range_frames"]
    assert r.source_channel_labels == want["source_channel_labels"]
    assert {e.name: [[c.name, c.marker] for c in e.channels] for e in r.experiments} == want["channels"]
    assert {e.name: e.channel_names for e in r.experiments} == want["channel_names"]
    assert {e.name: e.perturbation_wells for e in r.experiments} == want["perturbation_wells"]
    assert [e.name for e in r.subset(["expB"]).experiments] == want["subset"]
    assert r.get_experiment("expA").interval_minutes == 30.0
    with pytest.raises(KeyError, match="not found in registry"):
        r.get_experiment("expC")


@pytest.mark.parametrize("name", list(cases.INDEX_KW))
def test_index_anchors_clamped_centres_and_dropped_border_cells(golden, world, name):
    ix, want = make_index(world, **cases.INDEX_KW[name]), golden["index"][name]
    assert ix.max_border_shift == want["max_border_shift"]
    assert row_ids(ix.tracks) == want["tracks"]
    assert ix.tracks["y_clamp"].tolist() == want["y_clamp"] and ix.tracks["x_clamp"].tolist() == want["x_clamp"]
    assert row_ids(ix.valid_anchors) == want["valid_anchors"]
    assert ix.summary() == want["summary"]
    assert plain(ix.experiment_groups) == want["experiment_groups"] and plain(ix.condition_groups) == want["condition_groups"]


def test_index_border_policy(golden):
    """what the three settings must differ in: no shift drops every border cell, 3 keeps the cells at most 3 pixels off"""
    n = {k: len(golden["index"][k]["tracks"]) for k in ("temporal_no_shift", "temporal_shift_3", "temporal_default_shift")}
    assert n["temporal_no_shift"] < n["temporal_shift_3"] < n["temporal_default_shift"] < len(golden["table"]["cell_id"])


def test_index_needs_a_cell_index_and_clones(world):
    with pytest.raises(NotImplementedError, match="_load_all_experiments"):
        me.MultiExperimentIndex(registry=world["registry"], yx_patch_size=cases.YX_PATCH_SIZE)
    with pytest.raises(NotImplementedError, match="_reconstruct_lineage"):
        me.MultiExperimentIndex._reconstruct_lineage(None)
    ix = make_index(world)
    sub = ix.tracks[ix.tracks["experiment"] == "expB"]
    clone = ix.clone_with_subset(sub)
    assert len(clone.tracks) == len(sub) and set(clone.valid_anchors["experiment"].astype(str)) == {"expB"}
    assert clone.registry is ix.registry and clone.max_border_shift == ix.max_border_shift
    from_path = me.MultiExperimentIndex(registry=world["registry"], yx_patch_size=cases.YX_PATCH_SIZE,
                                        tau_range_hours=cases.TAU_RANGE_HOURS, cell_index_path=world["parquet"])
    assert row_ids(from_path.valid_anchors) == row_ids(ix.valid_anchors)


# ------------------------------------------------------------------------------------------------ dataset, host path
def forced_names(ds, n):
    if ds._channel_mode == "from_index":
        return [[ds._va_arrays["channel_name"][i]] for i in range(n)]
    return [ds._fixed_channel_names if ds._channel_mode == "fixed" else None] * n


@pytest.mark.parametrize("name", list(cases.DATASET_KW))
def test_dataset_boxes_targets_norm_meta_and_patches(golden, world, name):
    ds, want = make_dataset(world, **cases.DATASET_KW[name]), golden["dataset"][name]
    va = ds.index.valid_anchors
    assert row_ids(va) == want["valid_anchors"]
    forced = forced_names(ds, len(va))
    for i, rec in enumerate(want["boxes"]):
        box, norm = ds._slice_patch(ds._va_arrays, i, forced[i])
        got = [box.key[2], list(box.channels), box.z_start, box.z_start + box.z_count, box.y_start, box.y_start + box.y_count,
               box.x_start, box.x_start + box.x_count, *box.target]
        assert got == rec, i
        assert plain(norm) == want["norm_meta"][i], i
    for group, rec in want["patches"].items():
        boxes, _ = ds._slice_boxes(ds._va_arrays, rec["rows"], [forced[i] for i in rec["rows"]] if forced[0] is not None else None)
        got = ds._cut(boxes)
        assert got.dtype == torch.float32 and got.device.type == "cpu"
        assert torch.equal(got.view(torch.int32), rec["patches"].view(torch.int32)), (name, group)
    assert plain({k: {"column": c, "encoder": e} for k, (c, e) in ds._label_encoders.items()}) == want["label_encoders"]
    records = ds._extract_meta(va.iloc[want["meta"]["rows"]])
    for got, rec in zip(plain(records), want["meta"]["records"]):
        assert got.pop("store_path").endswith(rec["store_path"].rsplit("/", 1)[1])
        assert got == {k: v for k, v in rec.items() if k != "store_path"}


def test_mixed_channel_counts_raise_the_references_error(golden, world):
    ds = make_dataset(world, channels_per_sample=None)
    exp = ds.index.valid_anchors["experiment"].astype(str).to_numpy()
    rows = [int(np.flatnonzero(exp == "expA")[0]), int(np.flatnonzero(exp == "expB")[0])]
    with pytest.raises(RuntimeError) as err:
        ds.__getitems__(rows)
    assert str(err.value) == golden["dataset"]["all_channels"]["mixed_channel_error"]


@pytest.mark.parametrize("name", ["one_channel", "all_channels", "two_named"])
def test_norm_meta_from_the_positions_zattrs(golden, world, name):
    """a table without norm_* columns: statistics come from the FOV's ``normalization`` attribute, resolved to the row's time
    point, renamed to ``channel_0`` in the one-channel mode, ``None`` where the FOV has none"""
    bare = world["df"].drop(columns=[c for c in world["df"].columns if c.startswith("norm_")])
    ix = me.MultiExperimentIndex(registry=world["registry"], yx_patch_size=cases.YX_PATCH_SIZE,
                                 tau_range_hours=cases.TAU_RANGE_HOURS, cell_index_df=bare)
    ds = me.MultiExperimentTripletDataset(index=ix, tau_range_hours=cases.TAU_RANGE_HOURS, device="cpu", **cases.DATASET_KW[name])
    want = golden["zattrs_norm_meta"][name]
    assert row_ids(ix.valid_anchors) == want["valid_anchors"]
    forced = forced_names(ds, len(ix.valid_anchors))
    got = [plain(ds._build_norm_meta(ds._va_arrays, i, forced[i])) for i in range(len(ix.valid_anchors))]
    assert got == want["norm_meta"]
    assert any(m is None for m in got) and any(m is not None for m in got)


def test_null_norm_mean_falls_back_to_the_zattrs(golden, world):
    """norm_* columns present but null for expB (a float32 NaN after the parquet read): those rows take the FOV's attribute, the
    others keep the parquet's statistics.  (The reference hands the NaN on: INTEGRATION.md.)"""
    df = world["df"].copy()
    for col in ("norm_mean", "norm_std", "norm_median", "norm_iqr"):
        df.loc[df["experiment"] == "expB", col] = np.nan
    assert df["norm_mean"].dtype == np.float32
    ix = me.MultiExperimentIndex(registry=world["registry"], yx_patch_size=cases.YX_PATCH_SIZE,
                                 tau_range_hours=cases.TAU_RANGE_HOURS, cell_index_df=df)
    ds = me.MultiExperimentTripletDataset(index=ix, tau_range_hours=cases.TAU_RANGE_HOURS, device="cpu", channels_per_sample=1)
    n = len(ix.valid_anchors)
    got = [plain(ds._build_norm_meta(ds._va_arrays, i, [ds._va_arrays["channel_name"][i]])) for i in range(n)]
    from_parquet, from_zattrs = golden["dataset"]["one_channel"]["norm_meta"], golden["zattrs_norm_meta"]["one_channel"]["norm_meta"]
    exp = ix.valid_anchors["experiment"].astype(str).tolist()
    assert set(exp) == {"expA", "expB"}
    assert got == [from_zattrs[i] if e == "expB" else from_parquet[i] for i, e in enumerate(exp)]


def test_channel_tables_and_axis_tables_do_not_share_keys(world):
    """(4, 4, 6, 1) as a channel tuple equals the axis key (start 4, count 4, target 6, rescale True) of expA's Z table"""
    ds = make_dataset(world, channels_per_sample=1)
    box, _ = ds._slice_patch(ds._va_arrays, 0, ["Phase3D"])
    assert (box.z_start, box.z_count, box.target[0], box.scale != (1.0, 1.0, 1.0)) == (4, 4, 6, True)
    odd = me.PatchBox(**{**box.__dict__, "channels": (4, 4, 6, 1)})
    for first, second in ((box, odd), (odd, box)):
        ds._table_cache.clear(), ds._channel_tables.clear()
        ds._tables(first)
        chan, z, _, _ = ds._tables(second)
        assert chan.tolist() == list(second.channels) and z.tolist() == (4 + me.nearest_exact_index(4, 6)).tolist()


def test_predict_batches(golden, world):
    ds, want = make_dataset(world, index_kw=cases.INDEX_KW["predict"], fit=False, channels_per_sample=1), golden["predict"]
    batch = ds.__getitems__(want["rows"])
    assert sorted(batch) == want["keys"]
    assert plain(batch["index"]) == want["index"]
    assert torch.equal(batch["anchor"].view(torch.int32), want["anchor"].view(torch.int32))
    for got, rec in zip(plain(batch["anchor_meta"]), want["anchor_meta"]):
        got.pop("store_path"), rec.pop("store_path")
        assert got == rec


def test_dataset_refuses_what_is_not_built(world):
    with pytest.raises(NotImplementedError, match="return_negative"):
        make_dataset(world, return_negative=True)
    with pytest.raises(ValueError, match="must be 1"):
        make_dataset(world, channels_per_sample=2)
    with pytest.raises(TypeError, match="channels_per_sample"):
        make_dataset(world, channels_per_sample="Phase3D")
    with pytest.raises(NotImplementedError, match="__getitems__"):
        make_dataset(world, channels_per_sample=1)[0]


# ------------------------------------------------------------------------------------------------ positives
def test_temporal_positives_stay_in_the_lineage_the_marker_and_the_tau_window(world):
    ds = make_dataset(world, channels_per_sample=1)
    va, tr = ds.index.valid_anchors, ds.index.tracks
    ds._rng = np.random.default_rng(3)
    for _ in range(4):
        rows = list(range(len(va)))
        pos = ds._sample_positive_indices(rows)
        a, p = va.iloc[rows].reset_index(drop=True), tr.iloc[pos].reset_index(drop=True)
        assert (a["lineage_id"].astype(str) == p["lineage_id"].astype(str)).all()
        assert (a["experiment"].astype(str) == p["experiment"].astype(str)).all()
        assert (a["marker"].astype(str) == p["marker"].astype(str)).all()
        gap = (p["t"] - a["t"]).to_numpy()
        for g, exp in zip(gap, a["experiment"].astype(str)):
            lo, hi = world["registry"].tau_range_frames(exp, cases.TAU_RANGE_HOURS)
            assert lo <= g <= hi and g != 0
    batch = ds.__getitems__([0, 5, len(va) - 1])
    assert batch["anchor"].shape == batch["positive"].shape == (3, 1, 6, *cases.YX_PATCH_SIZE)
    assert [m["lineage_id"] for m in batch["anchor_meta"]] == [m["lineage_id"] for m in batch["positive_meta"]]
    assert len(batch["positive_norm_meta"]) == 3 and set(batch["positive_norm_meta"][0]) == {"channel_0"}


def test_column_match_positives_and_self_positives(world):
    cols = ["perturbation", "marker"]
    ds = make_dataset(world, index_kw=cases.INDEX_KW["match_columns"], channels_per_sample=1, positive_match_columns=cols)
    va, tr = ds.index.valid_anchors, ds.index.tracks
    rows = list(range(0, len(va), 3))
    pos = ds._sample_positive_indices(rows)
    for c in cols:
        assert (va.iloc[rows][c].astype(str).to_numpy() == tr.iloc[pos][c].astype(str).to_numpy()).all()
    ds = make_dataset(world, index_kw=cases.INDEX_KW["self"], channels_per_sample=1, positive_cell_source="self")
    batch = ds.__getitems__([1, 40, 90])
    assert torch.equal(batch["anchor"], batch["positive"]) and batch["anchor"].data_ptr() != batch["positive"].data_ptr()
    assert batch["positive_meta"] is batch["anchor_meta"] and batch["positive_norm_meta"] is batch["anchor_norm_meta"]
    assert not hasattr(ds, "_lineage_timepoints") and not hasattr(ds, "_match_lookup")   # nothing is looked up, nothing cut twice


# ------------------------------------------------------------------------------------------------ small pieces
def test_channel_dropout():
    x = torch.rand(6, 3, 2, 4, 4) + 1.0
    drop = me.ChannelDropout(channels=[1, 2], p=1.0)
    y = drop(x)
    assert bool((y[:, 1:] == 0).all()) and torch.equal(y[:, 0], x[:, 0]) and bool((x > 0).all())   # the input is left alone
    assert me.ChannelDropout(channels=[1], p=0.0)(x) is x
    assert drop.eval()(x) is x
    torch.manual_seed(0)
    half = me.ChannelDropout(channels=[0], p=0.5).train()(x)
    dropped = (half[:, 0].flatten(1) == 0).all(1)
    assert 0 < int(dropped.sum()) < 6 and torch.equal(half[~dropped], x[~dropped])


def test_parse_channel_name():
    assert me.parse_channel_name("Phase3D") == {"channel_type": "labelfree"}
    assert me.parse_channel_name("raw GFP EX488 EM525-45") == {"channel_type": "fluorescence", "filter_cube": "GFP",
                                                                "excitation_nm": 488, "emission_nm": 525}
    assert me.parse_channel_name("nuclei_prediction")["channel_type"] == "virtual_stain"
    assert me.parse_channel_name("BF_LED")["channel_type"] == "labelfree" and me.parse_channel_name("DIC")["channel_type"] == "labelfree"
    assert me.parse_channel_name("Cy5 EX640 EM680") == {"channel_type": "fluorescence", "excitation_nm": 640, "emission_nm": 680}
    assert me.parse_channel_name("TOMM20") == {"channel_type": "unknown"}


# ------------------------------------------------------------------------------------------------ module
def module_kw(world, **kw):
    base = dict(cell_index_path=world["parquet"], yx_patch_size=cases.YX_PATCH_SIZE, final_yx_patch_size=(8, 12),
                tau_range=cases.TAU_RANGE_HOURS, batch_size=6, seed=1, **cases.REGISTRY_KW)
    base.update(kw)
    return base


def test_config_resolves_the_class_path(world):
    from viscy_amd import config

    dm = config.instantiate({"class_path": "dynaclr.data.datamodule.MultiExperimentDataModule",
                             "init_args": module_kw(world, channels_per_sample=1, num_workers=4, pin_memory=True, buffer_size=4,
                                                    cache_pool_bytes=0, file_io_concurrency=2, recheck_cached_data="open",
                                                    prefetch_factor=2, device_cache_bytes=1 << 20)})
    assert type(dm) is me.MultiExperimentDataModule and dm.device_cache_bytes == 1 << 20 and dm.channel_dropout_channels == [1]


def test_fit_round_with_the_bag_of_channels_transforms_on_the_cpu(world):
    """sampler -> __getitems__ -> on_after_batch_transfer: (B, 1, z_window, *final_yx_patch_size); the Z reduction consumes the
    ``_is_labelfree`` mask (centre plane for the label-free samples, maximum for the others)"""
    from viscy_amd.transforms import BatchedChannelWiseZReductiond, NormalizeSampled

    seen = []

    class Spy(BatchedChannelWiseZReductiond):
        def _plan(self, data):
            seen.append(data["_is_labelfree"].clone())
            return super()._plan(data)

    dm = me.MultiExperimentDataModule(**module_kw(
        world, z_window=1, channels_per_sample=1, stratify_by="perturbation",
        normalizations=[NormalizeSampled(keys=["channel_0"], level="timepoint_statistics", subtrahend="mean", divisor="std")],
        augmentations=[Spy(keys=["channel_0"])]))
    dm.device = "cpu"
    dm.setup("fit")
    assert len(dm.train_dataset) > 0 and len(dm.val_dataset) > 0
    train_fovs = set(zip(dm.train_dataset.index.tracks["experiment"].astype(str), dm.train_dataset.index.tracks["fov_name"].astype(str)))
    val_fovs = set(zip(dm.val_dataset.index.tracks["experiment"].astype(str), dm.val_dataset.index.tracks["fov_name"].astype(str)))
    assert not train_fovs & val_fovs
    loader = dm.train_dataloader()
    assert isinstance(loader.batch_sampler, me.FlexibleBatchSampler) and loader.batch_sampler.seed == 1
    raw = next(iter(loader))
    assert raw["anchor"].shape == (6, 1, 6, *cases.YX_PATCH_SIZE)
    markers = [m["marker"] for m in raw["anchor_meta"]]
    centre = raw["anchor"][:, :, 3].clone()
    stats = raw["anchor_norm_meta"]
    batch = dm.on_after_batch_transfer(raw, 0)
    assert batch["anchor"].shape == batch["positive"].shape == (6, 1, 1, 8, 12)
    assert "anchor_norm_meta" not in batch and "positive_norm_meta" not in batch
    assert len(seen) == 2 and seen[0].tolist() == [m == "Phase3D" for m in markers]
    for b, marker in enumerate(markers):   # a label-free sample keeps the normalised centre plane
        if marker == "Phase3D":
            st = stats[b]["channel_0"]["timepoint_statistics"]
            want = ((centre[b] - st["mean"]) / st["std"])[:, 4:12, 4:16]
            assert torch.allclose(batch["anchor"][b, :, 0], want, rtol=1e-5, atol=1e-5)
    assert dm.val_dataloader() is not None


def test_experiment_split_predict_setup_and_mixed_norm_meta(world):
    dm = me.MultiExperimentDataModule(**module_kw(world, channels_per_sample=1, val_experiments=["expB"]))
    dm.device = "cpu"
    dm.setup("fit")
    assert set(dm.train_dataset.index.tracks["experiment"].astype(str)) == {"expA"}
    assert set(dm.val_dataset.index.tracks["experiment"].astype(str)) == {"expB"}
    with pytest.raises(ValueError, match="covers all experiments"):
        me.MultiExperimentDataModule(**module_kw(world, val_experiments=["expA", "expB"])).setup("fit")
    batch = dm.train_dataset.__getitems__([0, 1, 2])
    batch["anchor_norm_meta"][1] = None
    with pytest.raises(ValueError, match="Mixed None/non-None norm_meta in batch for 'anchor'"):
        dm.on_after_batch_transfer(batch, 0)
    dm.setup("predict")
    loader = dm.predict_dataloader()
    first = next(iter(loader))
    assert first["anchor"].shape == (6, 1, 6, *cases.YX_PATCH_SIZE) and len(first["index"]) == 6

    class Predicting:
        predicting = True

    dm.trainer = Predicting()
    out = dm.on_after_batch_transfer(first, 0)
    assert out["anchor"].shape == (6, 1, 4, 8, 12) and "anchor_meta" not in out and "index" in out
