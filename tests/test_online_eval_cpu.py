"""CPU: the host side of viscy_amd.online_eval — the stratified splits against sklearn's (tests/golden/online_eval.pt), pair order,
ranks and rho against scipy's, the float64 restatement against sklearn's predictions (the fixture's own check), the decisions of
``on_validation_epoch_end`` with the device functions replaced, the gather over a two-rank gloo group, the YAML seam and the
trainer's validation hooks."""

import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ref_online_eval as RO
from tests.conftest import load_golden
from viscy_amd import online_eval as OE


@pytest.fixture(scope="module")
def golden():
    return load_golden("online_eval.pt")


# ------------------------------------------------------------------------------------------------ splits
@pytest.mark.parametrize("name", list(RO.KNN_CASES))
def test_splits_are_sklearns(golden, name):
    c, g = RO.KNN_CASES[name], golden["knn"][name]
    _, y = RO.build_knn(name)
    if c["mode"] == "cv":
        assert g["folds"] == min(5, int(np.bincount(y).min()))
        ids = OE.stratified_kfold_ids(y, g["folds"])
    else:
        ids = OE.stratified_holdout_ids(y, RO.HOLDOUT_TEST_SIZE, seed=0)
        assert sorted(np.nonzero(ids == 1)[0]) == sorted(g["test_rows"].tolist())
        assert sorted(np.nonzero(ids == 0)[0]) == sorted(g["train_rows"].tolist())
    assert np.array_equal(ids, g["group"].numpy())


def test_three_fold_case_has_three_folds(golden):
    assert golden["knn"]["n131_d32_cv_3folds"]["folds"] == 3
    assert sorted(set(golden["knn"]["n131_d32_cv_3folds"]["group"].tolist())) == [0, 1, 2]


def test_splits_on_string_labels_and_errors():
    y = np.array(["b", "a", "b", "c", "a", "c", "b", "a", "c", "b"])
    codes = np.unique(y, return_inverse=True)[1]
    assert np.array_equal(OE.stratified_kfold_ids(y, 3), OE.stratified_kfold_ids(codes, 3))
    assert np.array_equal(OE.stratified_holdout_ids(y, 0.4), OE.stratified_holdout_ids(codes, 0.4))
    with pytest.raises(ValueError, match="only 1 member"):
        OE.stratified_holdout_ids(np.array([0, 0, 1, 1, 2]), 0.4)
    with pytest.raises(ValueError, match="n_splits"):
        OE.stratified_kfold_ids(np.array([0, 0, 1, 1]), 3)


# ------------------------------------------------------------------------------------------------ pairs, ranks, rho
@pytest.mark.parametrize("name", list(RO.SMOOTH_CASES))
def test_track_pairs_ranks_and_rho(golden, name):
    g = golden["smooth"][name]
    _, tid, t = RO.build_smooth(name)
    pi, pj = OE.track_pairs(tid)
    assert np.array_equal(pi, g["pi"].numpy()) and np.array_equal(pj, g["pj"].numpy())
    assert (tid[pi] == tid[pj]).all() and (pi < pj).all()
    if name == "two_pairs":
        assert len(pi) == 2 and np.isnan(g["fp64"])
        return
    assert len(pi) == 982
    dt = np.abs(t[pi] - t[pj]).astype(np.float64)
    d64 = g["dist64"].numpy()
    for ranks in (OE.average_ranks(dt), OE.average_ranks(torch.from_numpy(dt)).numpy()):
        assert np.array_equal(ranks, g["rank_dt"].numpy())       # many ties: |dt| takes 11 values
    assert np.array_equal(OE.average_ranks(torch.from_numpy(d64)).numpy(), g["rank_dist"].numpy())
    for rho in (OE.spearman_rho(dt, d64), OE.spearman_rho(torch.from_numpy(dt), torch.from_numpy(d64)), OE.spearman_rho(dt, torch.from_numpy(d64))):
        assert abs(rho - g["rho_scipy"]) <= 1e-12 and abs(rho - g["fp64"]) <= 1e-12
    assert 0.4 < g["fp64"] < 0.6
    assert np.isnan(OE.spearman_rho(np.ones(5), np.arange(5.0)))


def test_average_ranks_ties():
    assert OE.average_ranks(np.array([3.0, 1.0, 3.0, 2.0, 3.0])).tolist() == [4.0, 1.0, 4.0, 2.0, 4.0]
    assert OE.average_ranks(torch.tensor([0.5, 0.5])).tolist() == [1.5, 1.5]


def test_track_pairs_skips_singletons_and_handles_none():
    pi, pj = OE.track_pairs(np.array([5, 3, 5, 9, 3, 5]))
    assert list(zip(pi.tolist(), pj.tolist())) == [(1, 4), (0, 2), (0, 5), (2, 5)]   # track 3 first (np.unique order)
    pi, pj = OE.track_pairs(np.array([1, 2, 3]))
    assert len(pi) == 0 and len(pj) == 0


# ------------------------------------------------------------------------------------------------ the fixture's own check
@pytest.mark.parametrize("name", list(RO.KNN_CASES))
def test_restatement_reproduces_sklearn_on_decided_rows(golden, name):
    c, g = RO.KNN_CASES[name], golden["knn"][name]
    x, y = RO.build_knn(name)
    group = g["group"].numpy()
    pred, und = RO.undecided(x, y, group, g["k"])
    assert np.array_equal(und, g["undecided"].numpy())
    scored = np.ones(len(y), bool) if c["mode"] == "cv" else group == 1
    assert und[scored].mean() <= 0.02
    ok = scored & ~und
    assert np.array_equal(pred[ok], g["pred"].numpy()[ok])
    accs = [np.mean(pred[group == f] == y[group == f]) for f in (range(g["folds"]) if c["mode"] == "cv" else (1,))]
    assert abs(np.mean(accs) - g["acc"]) <= und[scored].sum() / scored.sum() + 1e-12


def test_restated_vote_ties_go_to_the_smallest_label():
    idx = np.array([[0, 1, 2, 3, 4, 5], [5, 4, 3, -1, -1, -1], [-1] * 6], dtype=np.int32)
    labels = np.array([7, 3, 7, 3, 5, 5])
    pred, margin = RO.knn_vote(idx, np.array([6, 3, 0]), labels)
    assert pred.tolist() == [3, 5, -1] and margin.tolist() == [0, 1, 0]   # a 3-way tie goes to 3; labels 5, 5, 3 vote 5


# ------------------------------------------------------------------------------------------------ decisions of the epoch end
class _Module:
    def __init__(self):
        self.logged = {}

    def _log(self, key, value):
        self.logged.setdefault(key, []).append(value)

    def __call__(self, x):
        return x.reshape(x.shape[0], -1)[:, :4].float(), None


class _Trainer:
    def __init__(self, epoch=0, sanity=False):
        self.current_epoch, self.sanity_checking, self.global_rank, self.world_size = epoch, sanity, 0, 1


def _run_epoch(cb, labels=None, tracks=None, times=None, epoch=0, n=None, label_key="marker", sanity=False):
    n = n if n is not None else len(labels)
    mod, tr = _Module(), _Trainer(epoch, sanity)
    cb.on_validation_epoch_start(tr, mod)
    for lo in range(0, n, 4):
        rows = range(lo, min(lo + 4, n))
        meta = []
        for r in rows:
            m = {}
            if labels is not None:
                m["labels"] = {label_key: labels[r]}
            if tracks is not None:
                m["global_track_id"] = tracks[r]
            if times is not None:
                m["t"] = times[r]
            meta.append(m)
        cb.on_validation_batch_end(tr, mod, None, {"anchor": torch.randn(len(rows), 1, 2, 2), "anchor_meta": meta}, lo // 4)
    cb.on_validation_epoch_end(tr, mod)
    return mod.logged


@pytest.fixture
def calls(monkeypatch):
    class Calls(list):
        rho = 0.25   # what the stand-in smoothness returns

    seen = Calls()

    def knn(features, labels, group, k, score_groups):
        seen.append(("knn", features.shape[0], np.asarray(labels).tolist(), np.asarray(group).tolist(), k, list(score_groups)))
        return 0.75

    monkeypatch.setattr(OE, "knn_accuracy", knn)
    monkeypatch.setattr(OE, "effective_rank", lambda f: seen.append(("erank", f.shape[0])) or 2.5)
    monkeypatch.setattr(OE, "temporal_smoothness", lambda f, tid, t: seen.append(("smooth", len(tid), len(t))) or seen.rho)
    return seen


def test_epoch_end_cv_path_and_reset(calls):
    cb = OE.OnlineEvalCallback(every_n_epochs=1, k=20)
    labels = [0, 1] * 6 + [2] * 3       # smallest class: 3 rows -> 3 folds; k = min(20, 15 - 1)
    logged = _run_epoch(cb, labels, tracks=list(range(15)), times=list(range(15)))
    assert logged == {"metrics/effective_rank/val": [2.5], "metrics/knn_acc/marker/val": [0.75], "metrics/temporal_smoothness/val": [0.25]}
    kind, n, y, group, k, scored = calls[1]
    assert (kind, n, y, k, scored) == ("knn", 15, labels, 14, [0, 1, 2])
    assert group == OE.stratified_kfold_ids(np.array(labels), 3).tolist()
    assert [c[0] for c in calls] == ["erank", "knn", "smooth"]
    assert not cb._collecting and cb._features == [] and cb._meta == []     # the reset


def test_epoch_end_bincount_quirk_and_degrade(calls):
    # labels 0 and 2: np.bincount counts 0 of label 1, so cv degrades to holdout, which needs 2 per class: no probe
    logged = _run_epoch(OE.OnlineEvalCallback(every_n_epochs=1), [0, 2] * 8)
    assert list(logged) == ["metrics/effective_rank/val"] and [c[0] for c in calls] == ["erank"]
    calls.clear()
    # a class of one row: cv -> holdout -> skipped; with every class >= 2 rows, explicit holdout runs and scores group 1 only
    assert list(_run_epoch(OE.OnlineEvalCallback(every_n_epochs=1), [0] * 8 + [1] * 7 + [2])) == ["metrics/effective_rank/val"]
    calls.clear()
    labels = [0] * 10 + [1] * 10
    logged = _run_epoch(OE.OnlineEvalCallback(every_n_epochs=1, knn_eval_mode="holdout", holdout_test_size=0.3, k=5, label_key="gene"),
                        labels, label_key="gene")
    assert logged["metrics/knn_acc/gene/val"] == [0.75]
    _, n, y, group, k, scored = calls[1]
    assert (n, k, scored) == (20, 5, [1]) and group == OE.stratified_holdout_ids(np.array(labels), 0.3, seed=0).tolist()
    assert sum(group) == 6


def test_epoch_end_skip_paths(calls):
    cb = OE.OnlineEvalCallback(every_n_epochs=1)
    assert list(_run_epoch(cb, None, n=8)) == ["metrics/effective_rank/val"]                      # no labels, no tracks
    assert list(_run_epoch(cb, [1] * 8)) == ["metrics/effective_rank/val"]                         # one unique label
    assert list(_run_epoch(cb, None, tracks=[1] * 8, n=8)) == ["metrics/effective_rank/val"]       # tracks without timepoints
    calls.rho = float("nan")
    assert list(_run_epoch(cb, None, tracks=[1] * 8, times=list(range(8)), n=8)) == ["metrics/effective_rank/val"]  # NaN is not logged
    # a label missing on one sample: the key counts as missing
    mod, tr = _Module(), _Trainer()
    cb.on_validation_epoch_start(tr, mod)
    cb.on_validation_batch_end(tr, mod, None, {"anchor": torch.randn(2, 1, 2, 2), "anchor_meta": [{"labels": {"marker": 0}}, {"labels": {}}]}, 0)
    cb.on_validation_epoch_end(tr, mod)
    assert list(mod.logged) == ["metrics/effective_rank/val"]
    # no batches at all
    cb.on_validation_epoch_start(tr, mod)
    cb.on_validation_epoch_end(tr, mod)
    assert not cb._collecting


def test_every_n_epochs_gate_and_sanity_check(calls):
    cb = OE.OnlineEvalCallback(every_n_epochs=5)
    assert _run_epoch(cb, [0, 1] * 4, epoch=3) == {} and calls == [] and cb._features == []
    assert _run_epoch(cb, [0, 1] * 4, epoch=5, sanity=True) == {}
    assert "metrics/knn_acc/marker/val" in _run_epoch(cb, [0, 1] * 4, epoch=5)
    assert calls[1][4] == 7   # k = min(20, 8 - 1)
    d = OE.OnlineEvalCallback()
    assert (d.every_n_epochs, d.label_key, d.k, d.track_id_key, d.timepoint_key, d.knn_eval_mode, d.holdout_test_size) == \
        (5, "marker", 20, "global_track_id", "t", "cv", 0.2)


def test_string_labels_are_encoded_before_the_bincount(calls):
    logged = _run_epoch(OE.OnlineEvalCallback(every_n_epochs=1), ["b", "a"] * 5)
    assert "metrics/knn_acc/marker/val" in logged
    assert calls[1][2] == [1, 0] * 5


def test_device_functions_have_no_cpu_fallback():
    x = torch.randn(8, 4)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        OE.knn_accuracy(x, [0, 1] * 4, [0, 0, 1, 1] * 2, 3, (0, 1))
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        OE.temporal_smoothness(x, [0] * 8, list(range(8)))
    with pytest.raises(ValueError, match="NaN or infinity"):
        OE.knn_accuracy(torch.full((8, 4), float("nan")), [0, 1] * 4, [0, 0, 1, 1] * 2, 3, (0, 1))
    assert np.isnan(OE.temporal_smoothness(x, [0, 0, 1, 1, 2, 3, 4, 5], list(range(8))))   # 2 pairs: NaN before any kernel


def test_effective_rank_edges():
    with pytest.warns(UserWarning, match="1/3 rows"):   # the non-finite row is dropped: the other two decide
        v = OE.effective_rank(torch.tensor([[3.0, 0.0], [float("nan"), 1.0], [0.0, 3.0]]))
    assert abs(v - 2.0) < 1e-12
    with pytest.warns(UserWarning, match="2/3 rows"):
        assert np.isnan(OE.effective_rank(torch.tensor([[float("inf"), 0.0], [float("nan"), 1.0], [0.0, 3.0]])))
    assert np.isnan(OE.effective_rank(torch.zeros(4, 3)))            # rank 0: no singular value above 1e-10
    assert np.isnan(OE.effective_rank(torch.ones(1, 3)))
    assert abs(OE.effective_rank(torch.eye(4)) - 4.0) < 1e-12        # four equal singular values
    assert abs(OE.effective_rank(torch.ones(5, 3)) - 1.0) < 1e-9     # complete collapse


# ------------------------------------------------------------------------------------------------ the gather, two ranks over gloo
def _gather_worker(rank, world, init_file, out):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    n = 5 if rank == 0 else 7                                   # unequal shards: both are cut to 5
    feats = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) + 100 * rank
    labels = np.array([f"r{rank}_{i}" for i in range(n)])      # strings: all_gather_object
    tracks = np.arange(n) + 10 * rank
    times = np.arange(n) if rank == 0 else None                 # one rank lacks the key: missing for all
    f, l, tr, ti = OE.OnlineEvalCallback._gather_across_ranks(feats, labels, tracks, times)
    out[rank] = (f, l.tolist(), tr.tolist(), ti)
    dist.destroy_process_group()


def test_gather_across_two_ranks():
    init_file = tempfile.mktemp()
    out = mp.Manager().dict()
    mp.spawn(_gather_worker, args=(2, init_file, out), nprocs=2, join=True)
    for rank in (0, 1):
        f, l, tr, ti = out[rank]
        want = torch.cat([torch.arange(15, dtype=torch.float32).reshape(5, 3), torch.arange(15, dtype=torch.float32).reshape(5, 3) + 100])
        assert torch.equal(f, want)
        assert l == [f"r0_{i}" for i in range(5)] + [f"r1_{i}" for i in range(5)]
        assert tr == [0, 1, 2, 3, 4, 10, 11, 12, 13, 14]
        assert ti is None


# ------------------------------------------------------------------------------------------------ the seams
def test_recipe_callback_list_instantiates_the_callback(golden):
    from viscy_amd import OnlineEvalCallback, config

    recipe = golden["recipe"]
    assert "viscy_utils.callbacks.OnlineEvalCallback" in [c["class_path"] for c in recipe["callbacks"]]
    skipped = []
    cbs = config.instantiate(recipe["callbacks"], skipped)
    assert [type(c) for c in cbs] == [OnlineEvalCallback] and OnlineEvalCallback is OE.OnlineEvalCallback
    assert (cbs[0].every_n_epochs, cbs[0].label_key, cbs[0].k) == (5, "perturbation", 20)
    assert sorted(skipped) == ["lightning.pytorch.callbacks.LearningRateMonitor", "lightning.pytorch.callbacks.ModelCheckpoint"]
    other = config.instantiate({"class_path": "viscy_utils.callbacks.online_eval.OnlineEvalCallback", "init_args": {"knn_eval_mode": "holdout"}})
    assert isinstance(other, OnlineEvalCallback) and other.knn_eval_mode == "holdout"


class _Recorder:
    def __init__(self):
        self.events = []

    def on_validation_epoch_start(self, trainer, module):
        self.events.append(("start", trainer.current_epoch, trainer.sanity_checking, trainer.global_rank, trainer.world_size))

    def on_validation_batch_end(self, trainer, module, outputs, batch, batch_idx, dataloader_idx=0):
        self.events.append(("batch", batch_idx, dataloader_idx, float(outputs), sorted(batch)))

    def on_validation_epoch_end(self, trainer, module):
        self.events.append(("end", trainer.current_epoch, list(module.events)))


class _TinyModule(torch.nn.Module):
    """a plain module with only the hooks a Lightning module must have"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.model = torch.nn.Identity()
        self.events = []

    def training_step(self, batch, i):
        return (self.w * batch["x"]).sum()

    def validation_step(self, batch, i, di=0):
        self.events.append(("val", i))
        return (self.w * batch["x"]).sum().detach()

    def on_validation_epoch_end(self):
        self.events.append("module_end")

    def configure_optimizers(self, t_total=None):
        return torch.optim.SGD(self.parameters(), lr=0.0)


class _TinyData:
    training = True

    def prepare_data(self):
        pass

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return [{"x": torch.ones(2)}]

    def val_dataloader(self):
        return [{"x": torch.ones(2)}, {"x": 2 * torch.ones(2)}]

    def on_after_batch_transfer(self, batch, di):
        return batch


def test_trainer_fit_calls_the_validation_hooks_in_order(monkeypatch):
    from viscy_amd.trainer import Trainer

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the hooks are host code: run the loop on the CPU
    rec = _Recorder()
    tr = Trainer(max_epochs=2, precision="32-true", callbacks=[rec])
    mod = _TinyModule()
    tr.fit(mod, _TinyData())
    per_epoch = len(rec.events) // 2
    assert per_epoch == 4
    e0 = rec.events[:4]
    assert e0[0] == ("start", 0, False, 0, 1)
    assert e0[1] == ("batch", 0, 0, 2.0, ["x"]) and e0[2] == ("batch", 1, 0, 4.0, ["x"])
    assert e0[3] == ("end", 0, [("val", 0), ("val", 1)])          # before the module's own on_validation_epoch_end
    assert rec.events[4][1] == 1 and rec.events[7][1] == 1
    assert mod.events.count("module_end") == 2
    Trainer(max_epochs=1, precision="32-true").fit(_TinyModule(), _TinyData())   # callbacks=[]: nothing to call
