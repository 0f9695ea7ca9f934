"""GPU: the kernels of csrc/online_eval.hip and viscy_amd.online_eval on top of them.

Exact contract.  Rows are small integers, so every dot product is an exact integer below 2^24 whatever the summation order, and
``inv`` is ones or powers of two, so fl32(fl32(dot * inv_i) * inv_j) has one value: idx, sim and cnt of vsx_knn_topk must be
bit-equal to the restatement (tests/ref_online_eval.py).  The fixtures repeat rows on purpose: most neighbour lists are decided
by the index rule alone.  Sizes sit on both sides of the 128-row query / candidate tile (and of its 64-column halves), of the
32-feature chunk and of the 4-float vector path (d % 4 != 0 takes scalar loads); N > 128 also runs the split / merge path.

sklearn cases.  Predictions equal sklearn's on every decided row; accuracy is within (undecided rows scored) / (rows scored) of
sklearn's (undecided: k-th / (k+1)-th similarity gap below d 2^-23 and vote margin below 3, see ref_online_eval.undecided).
Effective rank and smoothness: within the golden's margin 4 |reference fp32 - reference fp64| + 1e-9 of the reference's float64."""

import functools

import numpy as np
import pytest
import torch

from tests import ref_exact_tile as XT
from tests import ref_online_eval as RO
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("online_eval.pt")


def _groups(N, kind, seed):
    rng = np.random.RandomState(seed)
    if kind == "folds":          # three folds and a few rows that are nobody's candidate
        g = rng.randint(0, 3, N)
        g[rng.rand(N) < 0.1] = -1
    elif kind == "few":          # rows of group 0 have at most 4 candidates: cnt < k, padded slots
        g = np.zeros(N, dtype=np.int64)
        g[rng.permutation(N)[: min(4, N - 1)]] = 1
    else:                        # "one": a single group, no candidates at all
        g = np.full(N, 2)
    return g.astype(np.int32)


def _inv(N, kind, seed):
    if kind == "ones":
        return np.ones(N, dtype=np.float32)
    return (2.0 ** -np.random.RandomState(seed).randint(0, 4, N)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _exact_case(N, d, k, gkind, ikind):
    """inputs and the restatement's answer, once per case; never written to"""
    seed = 1000 * N + 10 * d + k
    x = RO.integer_rows(N, d, seed)
    group, inv = _groups(N, gkind, seed + 1), _inv(N, ikind, seed + 2)
    idx, sim, cnt, _ = RO.knn_topk(RO.similarity(x, inv, exact32=True), group, k)
    return x, inv, group, idx, sim, cnt


def _raw_topk(x, inv, group, k, x_offset=0):
    """vsx_knn_topk on buffers pre-filled with sentinels (and a workspace full of junk): every slot must be written.
    x_offset: the rows start that many floats past a 16-byte boundary"""
    from viscy_amd import _lib

    L = _lib.lib()
    N, d = x.shape
    xd, invd, gd = (torch.from_numpy(a).to(DEV) for a in (x, inv, group))
    if x_offset:
        buf = torch.empty(N * d + x_offset, dtype=torch.float32, device=DEV)
        buf[x_offset:].copy_(xd.view(-1))
        xd = buf[x_offset:].view(N, d)
        assert buf.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 4 * x_offset % 16 != 0 and xd.is_contiguous()
    idx = torch.full((N, k), -7, dtype=torch.int32, device=DEV)
    sim = torch.full((N, k), 123.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    nbytes = L.vsx_knn_topk_ws_bytes(N, d, k)
    assert 0 < nbytes <= 8 * N * (8 * k + 4)          # O(N k): no N x N term
    ws = torch.full(((nbytes + 3) // 4,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    rc = L.vsx_knn_topk(xd.data_ptr(), invd.data_ptr(), gd.data_ptr(), N, d, k, idx.data_ptr(), sim.data_ptr(), cnt.data_ptr(),
                        ws.data_ptr(), ws.numel() * 4, _lib.stream())
    assert rc == 0, L.vsx_last_error()
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sim.cpu().numpy(), cnt.cpu().numpy()


EXACT = [
    # N around 1, the 64-column half, the 128-row tile, two and three tiles; d = 1, 3 (scalar loads), 4, 33 (chunk + 1), 768
    (1, 4, 1, "folds", "ones"), (5, 3, 7, "folds", "pow2"), (5, 1, 1, "folds", "ones"),
    (63, 4, 20, "folds", "pow2"), (64, 33, 7, "folds", "ones"), (65, 1, 64, "folds", "pow2"),
    (127, 3, 20, "folds", "ones"), (128, 4, 64, "folds", "pow2"), (129, 33, 1, "folds", "ones"),
    (255, 33, 20, "folds", "pow2"), (256, 768, 7, "folds", "ones"), (257, 4, 20, "folds", "pow2"),
    (300, 768, 20, "folds", "pow2"), (385, 3, 64, "folds", "ones"),
    # fewer than k candidates; none
    (65, 4, 7, "few", "pow2"), (257, 33, 20, "few", "ones"), (130, 4, 64, "few", "pow2"),
    (5, 4, 7, "one", "ones"), (129, 3, 20, "one", "pow2"),
    # two and three candidate tiles per workgroup (tests/ref_exact_tile.KNN_CASES states each leg), one case per KB instance:
    # KB 8 on scalar loads; KB 24 with a shorter last split; KB 64 with three tiles per split; cnt < k carried across tiles
    (1153, 3, 7, "folds", "ones"), (1030, 4, 20, "folds", "pow2"), (2171, 33, 64, "folds", "pow2"), (1030, 4, 20, "few", "pow2"),
]
MULTI_TILE = [c["case"] for c in XT.KNN_CASES]


def _assert_two_tiles_per_workgroup(N):
    """the leg with the device's own compute-unit count; a device that gives these sizes one tile per workgroup fails here"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert XT.knn_plan(N, cus)[2] >= 2, (N, cus, XT.knn_leg(N, cus))


@pytest.mark.parametrize("N,d,k,gkind,ikind", EXACT, ids=[f"N{c[0]}_d{c[1]}_k{c[2]}_{c[3]}_{c[4]}" for c in EXACT])
def test_knn_topk_is_bit_equal_to_the_restatement(N, d, k, gkind, ikind):
    x, inv, group, idx_r, sim_r, cnt_r = _exact_case(N, d, k, gkind, ikind)
    if (N, d, k, gkind, ikind) in MULTI_TILE:
        _assert_two_tiles_per_workgroup(N)
    idx, sim, cnt = _raw_topk(x, inv, group, k)
    assert np.array_equal(cnt, cnt_r)
    assert np.array_equal(idx, idx_r)
    assert np.array_equal(sim.view(np.int32), sim_r.view(np.int32))            # bit for bit, -inf padding included
    if gkind == "folds" and N >= 63:
        full = cnt_r == k
        ties = (sim_r[full, :-1] == sim_r[full, 1:]).mean() if k > 1 and full.any() else 1.0
        assert ties > 0.2, ties                                                  # the index rule is what is being tested
    if gkind == "few":
        assert (cnt_r[group == 0] == min(4, N - 1)).all() and (idx_r[group == 0, min(4, N - 1):] == -1).all()
    if gkind == "one":
        assert (cnt == 0).all() and (idx == -1).all() and np.isneginf(sim).all()


def test_knn_topk_on_rows_off_the_16_byte_grid():
    """d % 4 == 0 but x only 4-byte aligned: ft_vec_ok is false and the rows come feature by feature; same bits, two tiles per
    workgroup"""
    N, d, k, gkind, ikind = XT.KNN_VIEW_CASE
    assert XT.KNN_VIEW_CASE in EXACT
    x, inv, group, idx_r, sim_r, cnt_r = _exact_case(N, d, k, gkind, ikind)
    _assert_two_tiles_per_workgroup(N)
    idx, sim, cnt = _raw_topk(x, inv, group, k, x_offset=1)
    assert np.array_equal(cnt, cnt_r) and np.array_equal(idx, idx_r) and np.array_equal(sim.view(np.int32), sim_r.view(np.int32))


def test_knn_topk_refuses_what_it_does_not_serve():
    from viscy_amd import _lib, ops

    L = _lib.lib()
    x = torch.zeros(8, 4, device=DEV)
    inv, group = torch.ones(8, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    out_i, out_s, out_c = torch.zeros(8, 65, dtype=torch.int32, device=DEV), torch.zeros(8, 65, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    for k in (65, 0):
        rc = L.vsx_knn_topk(x.data_ptr(), inv.data_ptr(), group.data_ptr(), 8, 4, k, out_i.data_ptr(), out_s.data_ptr(), out_c.data_ptr(),
                            ws.data_ptr(), ws.numel() * 4, _lib.stream())
        assert rc != 0 and b"k=%d must be in [1, 64]" % k in L.vsx_last_error()
        assert L.vsx_knn_topk_ws_bytes(8, 4, k) == 0
    rc = L.vsx_knn_topk(x.data_ptr(), inv.data_ptr(), group.data_ptr(), 8, 4, 7, out_i.data_ptr(), out_s.data_ptr(), out_c.data_ptr(),
                        ws.data_ptr(), 16, _lib.stream())
    assert rc != 0 and b"workspace" in L.vsx_last_error()                       # too small a workspace is refused, not overrun
    with pytest.raises(ValueError, match="k=65"):
        ops.knn_topk(x, inv, group, 65)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.knn_topk(x.cpu(), inv, group, 3)


def test_ops_knn_topk_matches_the_raw_call():
    from viscy_amd import ops

    x, inv, group, idx_r, sim_r, cnt_r = _exact_case(257, 4, 20, "folds", "pow2")
    idx, sim, cnt = ops.knn_topk(*(torch.from_numpy(a).to(DEV) for a in (x, inv, group)), 20)
    assert np.array_equal(idx.cpu().numpy(), idx_r) and np.array_equal(sim.cpu().numpy(), sim_r) and np.array_equal(cnt.cpu().numpy(), cnt_r)


@pytest.mark.parametrize("N,d,k", [(130, 36, 64), XT.KNN_ORDER_CASE])
def test_knn_similarities_are_the_classifier_heads_logits_bit_for_bit(N, d, k):
    """csrc/f32_tile.h promises ONE summation order of a dot product for every kernel built on it.  On float rows (integer rows
    cannot see a reordered sum) a similarity of vsx_knn_topk and a cosine logit of vsx_cls_logits over the same two rows are
    both fl32(fl32(dot * inv_i) * inv_j) — times expf(0) = 1 on the head's side — so only the dot's order could tell them apart.
    N = 130, d = 36: two tiles in each direction, the 64-column half boundary, one chunk plus one float4.  N = 1030: nine tiles,
    two per workgroup of the probe, so the order also holds for the second tile a workgroup forms."""
    from viscy_amd import ops

    if N > 130:
        _assert_two_tiles_per_workgroup(N)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(100 * N + d)).to(DEV)
    inv = ops.row_inv_norm(x, 0.0)
    group = (torch.arange(N, dtype=torch.int32) % 3).to(DEV)
    idx, sim, cnt = ops.knn_topk(x, inv, group, k)
    Z = ops.cls_logits(x, x, inv_h=inv, inv_w=inv, log_scale=torch.zeros(1, device=DEV))
    assert (cnt == k).all()                                                       # every row has at least 86 candidates (N = 130)
    used = torch.arange(k, device=DEV)[None, :] < cnt[:, None]
    logit = Z.gather(1, idx.clamp_min(0).long())
    assert torch.equal(sim.view(torch.int32)[used], logit.view(torch.int32)[used])


def test_knn_vote_against_the_restatement():
    from viscy_amd import ops

    rng = np.random.RandomState(5)
    N, k, C = 200, 20, 100                                  # more classes than neighbours
    labels = rng.randint(0, C, 500).astype(np.int32)
    labels[:6] = [7, 3, 7, 3, 5, 5]
    idx = rng.randint(0, 500, (N, k)).astype(np.int32)
    cnt = rng.randint(0, k + 1, N).astype(np.int32)
    idx[0, :6], cnt[0] = [0, 1, 2, 3, 4, 5], 6              # a three-way tie 7 / 3 / 5: the smallest label wins
    idx[1, :3], cnt[1] = [5, 4, 3], 3
    cnt[2], cnt[3] = 0, k
    idx[np.arange(k)[None, :] >= cnt[:, None]] = -1
    want, _ = RO.knn_vote(idx, cnt, labels)
    assert want[0] == 3 and want[1] == 5 and want[2] == -1
    got = ops.knn_vote(torch.from_numpy(idx).to(DEV), torch.from_numpy(cnt).to(DEV), torch.from_numpy(labels).to(DEV))
    assert np.array_equal(got.cpu().numpy(), want)
    # few classes: long runs of equal labels, ties between the two or three of them
    labels2 = rng.randint(0, 3, 500).astype(np.int32)
    idx64, cnt64 = rng.randint(0, 500, (130, 64)).astype(np.int32), np.full(130, 64, dtype=np.int32)
    want2, _ = RO.knn_vote(idx64, cnt64, labels2)
    got2 = ops.knn_vote(torch.from_numpy(idx64).to(DEV), torch.from_numpy(cnt64).to(DEV), torch.from_numpy(labels2).to(DEV))
    assert np.array_equal(got2.cpu().numpy(), want2)


@pytest.mark.parametrize("N,d", [(1, 1), (5, 3), (130, 33), (257, 768)])
def test_row_inv_norm_with_a_zero_row(N, d):
    from viscy_amd import ops

    x = np.random.RandomState(N + d).randn(N, d).astype(np.float32)
    x[N // 2] = 0.0
    xd = torch.tensor(x, device=DEV)
    # fp32 sum of d non-negative terms: relative error <= (d - 1) u, halved by the square root; the add, the root and the
    # division round once each: (d / 2 + 3) u, u = 2^-24
    tol = (d / 2 + 3) * 2.0 ** -24
    for eps in (0.0, 1e-10):
        got = ops.row_inv_norm(xd, eps).cpu().numpy().astype(np.float64)
        want = RO.inv_norm(x, eps)
        if eps == 0.0:
            assert got[N // 2] == 0.0 and want[N // 2] == 0.0      # sklearn's normalize leaves a zero row zero
        else:
            assert got[N // 2] == np.float32(1.0) / np.float32(1e-10)
        rest = np.arange(N) != N // 2
        assert (np.abs(got[rest] - want[rest]) <= tol * want[rest]).all()


def test_pair_cosine_dist_on_the_integer_fixture():
    from viscy_amd import ops

    for N, d in ((65, 33), (130, 768), (9, 1)):
        x, inv = RO.integer_rows(N, d, 77 + d), _inv(N, "pow2", 78 + d)
        rng = np.random.RandomState(d)
        pi, pj = rng.randint(0, N, 333).astype(np.int32), rng.randint(0, N, 333).astype(np.int32)
        dot = (x[pi].astype(np.float64) * x[pj].astype(np.float64)).sum(1).astype(np.float32)
        want = np.float32(1.0) - (dot * inv[pi]) * inv[pj]
        got = ops.pair_cosine_dist(*(torch.from_numpy(a).to(DEV) for a in (x, inv, pi, pj)))
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32))
    assert ops.pair_cosine_dist(torch.ones(3, 2, device=DEV), torch.ones(3, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                torch.zeros(0, dtype=torch.int32, device=DEV)).numel() == 0


@pytest.mark.parametrize("name", list(RO.KNN_CASES))
def test_knn_accuracy_against_sklearn(name):
    from viscy_amd import online_eval as OE

    c, g = RO.KNN_CASES[name], golden()["knn"][name]
    x, y = RO.build_knn(name)
    group = g["group"].numpy()
    xd = torch.tensor(x, device=DEV)
    if c["mode"] == "cv":
        scored, score_groups = np.ones(len(y), bool), range(g["folds"])
        assert np.array_equal(OE.stratified_kfold_ids(y, g["folds"]), group)
    else:
        scored, score_groups = group == 1, (1,)
        assert np.array_equal(OE.stratified_holdout_ids(y, RO.HOLDOUT_TEST_SIZE), group)
    pred, y_d, classes = OE.knn_predict(xd, y, group, g["k"])
    pred = classes[pred.cpu().numpy()]
    und = g["undecided"].numpy()
    decided = scored & ~und
    differ = int((pred[decided] != g["pred"].numpy()[decided]).sum())
    acc = OE.knn_accuracy(xd, y, group, g["k"], score_groups)
    bound = und[scored].sum() / scored.sum()
    print(f"{name}: accuracy {acc:.6f} sklearn {g['acc']:.6f} |diff| {abs(acc - g['acc']):.2e} bound {bound:.2e}; "
          f"{differ} decided rows differ; {int((pred[scored] != g['pred'].numpy()[scored]).sum())} scored rows differ")
    assert differ == 0
    assert abs(acc - g["acc"]) <= bound + 1e-12


def test_knn_accuracy_refuses_non_finite_features():
    from viscy_amd import online_eval as OE

    x = torch.randn(16, 8, device=DEV)
    x[3, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or infinity"):
        OE.knn_accuracy(x, [0, 1] * 8, [0, 0, 1, 1] * 4, 3, (0, 1))


@pytest.mark.parametrize("name", RO.ERANK_CASES)
def test_effective_rank_against_the_reference(name):
    from viscy_amd import online_eval as OE

    g = golden()["erank"][name]
    x, _ = RO.build_knn(name)
    got = OE.effective_rank(torch.tensor(x, device=DEV))
    print(f"effective_rank {name}: {got:.12f} reference fp64 {g['fp64']:.12f} |diff| {abs(got - g['fp64']):.2e} margin {g['margin']:.2e}")
    assert abs(got - g["fp64"]) <= g["margin"]


def test_effective_rank_drops_non_finite_rows_on_the_device():
    from viscy_amd import online_eval as OE

    x, _ = RO.build_knn("n130_d33_cv")
    xd = torch.tensor(x, device=DEV)
    bad = torch.cat([xd[:50], torch.full((1, 33), float("nan"), device=DEV), xd[50:]])
    with pytest.warns(UserWarning, match="1/131 rows"):
        assert OE.effective_rank(bad) == OE.effective_rank(xd)
    assert np.isnan(OE.effective_rank(xd[:1]))


def test_temporal_smoothness_against_the_reference():
    from viscy_amd import online_eval as OE

    g = golden()["smooth"]["tracks40"]
    x, tid, t = RO.build_smooth("tracks40")
    got = OE.temporal_smoothness(torch.tensor(x, device=DEV), tid, t)
    print(f"temporal_smoothness: {got:.12f} reference fp64 {g['fp64']:.12f} |diff| {abs(got - g['fp64']):.2e} margin {g['margin']:.2e}")
    assert abs(got - g["fp64"]) <= g["margin"]
    x2, tid2, t2 = RO.build_smooth("two_pairs")
    assert np.isnan(golden()["smooth"]["two_pairs"]["fp64"]) and np.isnan(OE.temporal_smoothness(torch.tensor(x2, device=DEV), tid2, t2))


# ------------------------------------------------------------------------------------------------ end to end
class _Batches:
    """a list-of-batches datamodule: ``anchor`` / ``positive`` / ``anchor_meta`` as a TripletDataModule hands them over"""
    training = True

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.train = [self._batch(g, 4, 0)]
        self.val = [self._batch(g, 6, 6 * i) for i in range(4)]     # 24 rows: 3 labels x 8, 6 tracks x 4 timepoints

    @staticmethod
    def _batch(g, b, row0):
        a = torch.randn(b, 1, 5, 64, 64, generator=g)
        meta = [{"labels": {"marker": (row0 + r) % 3}, "global_track_id": (row0 + r) % 6, "t": (row0 + r) // 6} for r in range(b)]
        return {"anchor": a, "positive": a + 0.3 * torch.randn(a.shape, generator=g), "anchor_meta": meta}

    def prepare_data(self):
        pass

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return self.train

    def val_dataloader(self):
        return self.val

    def on_after_batch_transfer(self, batch, dataloader_idx):
        return batch


def _fit_once():
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule
    from viscy_amd.online_eval import OnlineEvalCallback
    from viscy_amd.trainer import Trainer

    torch.manual_seed(0)
    enc = ContrastiveEncoder("convnext_tiny", in_channels=1, in_stack_depth=5, embedding_dim=64, projection_dim=32,
                             depths=(1, 1, 2, 1), dims=(32, 64, 96, 128))
    # lr = 0: the run-to-run comparison below is about the callback, not about the order of the backward pass's sums
    mod = ContrastiveModule(enc, lr=0.0).cuda()
    enc.compute_dtype = torch.float32
    dm = _Batches()
    Trainer(max_epochs=1, precision="32-true", seed=0, callbacks=[OnlineEvalCallback(every_n_epochs=1, k=5)]).fit(mod, dm)
    return mod, dm


def test_fit_logs_the_three_metrics_and_they_are_the_device_functions_values():
    from viscy_amd import online_eval as OE

    mod, dm = _fit_once()
    keys = ["metrics/effective_rank/val", "metrics/knn_acc/marker/val", "metrics/temporal_smoothness/val"]
    assert all(len(mod.logged[k]) == 1 for k in keys), sorted(mod.logged)
    mod.eval()
    with torch.no_grad():
        feats = torch.cat([mod(b["anchor"].cuda())[0] for b in dm.val]).float()
    meta = [m for b in dm.val for m in b["anchor_meta"]]
    labels = np.array([m["labels"]["marker"] for m in meta])
    tracks, times = np.array([m["global_track_id"] for m in meta]), np.array([m["t"] for m in meta])
    assert feats.shape == (24, 128) and feats.is_cuda   # the trunk's width: dims[-1]
    want = {keys[0]: OE.effective_rank(feats),
            keys[1]: OE.knn_accuracy(feats, labels, OE.stratified_kfold_ids(labels, 5), 5, range(5)),
            keys[2]: OE.temporal_smoothness(feats, tracks, times)}
    got = {k: mod.logged[k][0] for k in keys}
    print("online eval, end to end:", got)
    assert got == want
    assert 1.0 <= got[keys[0]] <= 24.0 and 0.0 <= got[keys[1]] <= 1.0 and -1.0 <= got[keys[2]] <= 1.0
    again, _ = _fit_once()
    assert {k: again.logged[k][0] for k in keys} == got      # bit-identical from run to run
