"""CPU: the host half of viscy_amd.clustering and the fixtures the GPU tests (tests/test_gpu_clustering.py) stand on.

* the reference's own matrices (tests/golden/clustering.pt) lie inside the bounds of tests/ref_clustering.py: cosine within
  4 (d + 8) u of the long-double truth, Euclidean compared on d^2 within 2 (d + 8) u (n_i + n_j) of the difference-form truth
  (plus the 2 u d^2 of its square root);
* the numpy restatement reproduces every golden value: sklearn's DBSCAN labels from the order-free rule, its k-NN accuracy from
  the (distance, index) order, NMI (within (R C + 16) u) and ARI (equal) of viscy_amd.clustering's host functions and of the
  long-double restatement on 40 seeded labelings, the stable ranks wherever a row has no ties;
* the real-valued fixtures meet their two conditions, and the lattice fixtures do have pairs at exactly eps;
* ranks, block selection, time offsets and every refusal that needs no device."""

import functools

import numpy as np
import pytest
import torch

from tests import ref_clustering as RC
from tests.conftest import load_golden
from viscy_amd import clustering as CL


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("clustering.pt")


def test_golden_holds_results_only():
    g = golden()
    assert set(g) == {"numpy", "scipy", "sklearn", "torch", "dist", "ranks", "dbscan", "eval", "knn", "scores", "errors", "seeds"}
    assert set(g["dist"]) == set(RC.DISTANCE_CASES) and set(g["ranks"]) == set(RC.RANK_CASES)
    assert set(g["dbscan"]) == set(RC.dbscan_cases()) and set(g["knn"]) == set(RC.knn_cases())
    assert g["seeds"] == {d: RC.blob_case(d)[0] for d in (16, 768)}
    assert g["errors"]["method"] == ("ValueError", "Invalid method. Choose 'nmi' or 'ari'.")
    assert g["errors"]["k_above_n"][0] == "ValueError" and g["errors"]["k_above_n"][1].startswith("Expected n_neighbors <= n_samples_fit")


@pytest.mark.parametrize("name", RC.DISTANCE_CASES)
def test_reference_matrices_lie_inside_the_bounds(name):
    x = RC.distance_case(name)
    g = golden()["dist"][name]
    cos, eu = g["cosine"].numpy(), g["euclidean"].numpy()
    assert cos.dtype == eu.dtype == np.float64 and cos.shape == eu.shape == (len(x), len(x))
    errc = np.abs(cos - RC.cosine_truth(x))
    err2 = np.abs(eu ** 2 - RC.sqdist_truth(x))
    bound2 = RC.sqdist_bound(x) + 2 * RC.U * eu ** 2
    print(f"{name}: cosine {errc.max() / RC.U:.1f} u of {RC.cosine_bound(x) / RC.U:.0f} u; d2 error / bound {np.max(err2 / np.maximum(bound2, 1e-300)):.4f}")
    assert (errc <= RC.cosine_bound(x)).all()
    assert (err2 <= bound2).all()
    # the restatement is the module's contract: the truth with an exact zero diagonal
    for metric, ref in (("cosine", cos), ("euclidean", eu)):
        mine = RC.pairwise_distance_matrix(x, metric)
        assert (np.diag(mine) == 0.0).all() and np.allclose(mine[RC.off_diagonal(len(x))], ref[RC.off_diagonal(len(x))], rtol=0, atol=1e-5)


def test_lattice_features_are_exact():
    x = RC.distance_case("lattice_50x7")
    assert np.abs(x).max() <= 512 and (x == np.rint(x)).all()
    d2 = RC.sqdist_truth(x)
    assert (d2 == np.rint(d2)).all()
    eu = golden()["dist"]["lattice_50x7"]["euclidean"].numpy()
    assert (np.abs(eu - np.sqrt(d2)) <= 2 * RC.U * eu).all()      # the reference's small-N cdist path: within an ulp of np.sqrt


@pytest.mark.parametrize("name", RC.RANK_CASES)
def test_stable_ranks_against_the_reference(name):
    g = golden()
    eu = g["dist"][name]["euclidean"].numpy()
    raw, norm = g["ranks"][name]["raw"].numpy(), g["ranks"][name]["norm"].numpy()
    mine = CL.rank_nearest_neighbors(eu, normalize=False)
    assert mine.dtype == np.int64 and np.array_equal(mine, RC.rank_nearest_neighbors(eu, False))
    untied = np.array([len(np.unique(row)) == len(row) for row in eu])
    assert untied.all() == (name != "real_20x3")                  # its three duplicate rows tie in every row
    assert np.array_equal(mine[untied], raw[untied])
    mine_n = CL.rank_nearest_neighbors(eu, normalize=True)
    assert mine_n.dtype == np.float64 and np.array_equal(mine_n[untied], norm[untied])
    for row, r in zip(eu, mine):                                   # a permutation that sorts the row, ties to the lower index
        order = np.empty(len(row), dtype=np.int64)
        order[r] = np.arange(len(row))
        assert sorted(r) == list(range(len(row))) and (np.diff(row[order]) >= 0).all()
        assert all(order[i] < order[i + 1] for i in range(len(row) - 1) if row[order[i]] == row[order[i + 1]])
    t = CL.rank_nearest_neighbors(torch.from_numpy(eu), normalize=False)
    assert torch.is_tensor(t) and t.dtype == torch.int64 and np.array_equal(t.numpy(), mine)
    assert CL.rank_nearest_neighbors(torch.from_numpy(eu)).dtype == torch.float64


def test_select_block_and_time_offset():
    m = np.arange(36.0).reshape(6, 6)
    idx = np.array([4, 1, 5])
    assert np.array_equal(CL.select_block(m, idx), m[np.ix_(idx, idx)])
    assert np.array_equal(CL.compare_time_offset(m), np.array([6.0, 13.0, 20.0, 27.0, 34.0]))
    assert np.array_equal(CL.compare_time_offset(m, time_offset=4), np.array([24.0, 31.0]))


@pytest.mark.parametrize("name", sorted(RC.dbscan_cases()))
def test_order_free_rule_gives_sklearns_labels(name):
    x, eps, min_samples = RC.dbscan_cases()[name]
    want = golden()["dbscan"][name].numpy()
    d2 = RC.sqdist_truth(x)
    assert np.array_equal(RC.dbscan(d2, eps * eps, min_samples), want)
    if name.startswith("blobs"):
        assert RC.eps_margin_ok(x, eps)
    else:
        assert (x == np.rint(x)).all() and np.abs(x).max() <= 512
        assert (d2[RC.off_diagonal(len(x))] == eps * eps).sum() > 0            # pairs at exactly eps
    adj, deg = RC.graph_bits(d2, eps * eps)
    assert adj.dtype == np.uint64 and adj.shape == (len(x), -(-len(x) // 64))
    assert [sum(bin(int(w)).count("1") for w in row) for row in adj] == list(deg)


def test_dbscan_fixtures_say_what_they_claim():
    g = golden()["dbscan"]
    assert (g["chain"].numpy() == 0).all() and len(g["chain"]) == 3 * 64 + 5
    sb = g["shared_border_4"].numpy()
    assert sb[0] == 0 and set(sb[1:5]) == {0} and set(sb[5:]) == {1}           # two clusters; the border point takes the lower
    assert np.array_equal(g["shared_border_5"].numpy(), sb)                    # exactly min_samples neighbours: core
    assert (g["all_noise"].numpy() == -1).all()                                # one fewer: not core
    assert g["lattice_2d_min1"].numpy().min() == 0                             # min_samples = 1: no noise
    for d in (16, 768):
        lab = g["blobs_%d" % d].numpy()
        assert lab.max() == 2 and (lab == -1).sum() == 5


@pytest.mark.parametrize("d", [16, 768])
def test_blob_fixture_conditions_and_scores(d):
    seed, (x, y, noisy) = RC.blob_case(d)
    assert x.dtype == np.float32 and x.shape == (140, d)
    assert RC.eps_margin_ok(x, 0.5) and RC.knn_margin_ok(x, noisy, RC.KNN_K)
    assert seed == golden()["seeds"][d]
    clusters = golden()["dbscan"]["blobs_%d" % d].numpy()
    want = golden()["eval"]["blobs_%d" % d]
    bound = RC.nmi_bound(len(np.unique(noisy)), len(np.unique(clusters)))
    assert abs(CL.normalized_mutual_info(noisy, clusters) - want["nmi"]) <= bound and abs(RC.nmi(noisy, clusters) - want["nmi"]) <= bound
    assert CL.adjusted_rand(noisy, clusters) == want["ari"] == RC.ari(noisy, clusters)
    assert 0.3 < want["nmi"] < 0.9


def test_nmi_and_ari_against_sklearn_on_seeded_labelings():
    pairs, scores = RC.random_labelings(), golden()["scores"]
    assert len(pairs) == len(scores) == 40
    worst = 0.0
    for (a, b), (nmi, ari) in zip(pairs, scores):
        bound = RC.nmi_bound(len(np.unique(a)), len(np.unique(b)))
        got = CL.normalized_mutual_info(a, b)
        worst = max(worst, abs(got - nmi) / RC.U)
        assert abs(got - nmi) <= bound and abs(RC.nmi(a, b) - nmi) <= bound, (got, nmi)
        assert CL.adjusted_rand(a, b) == ari == RC.ari(a, b)
    print(f"NMI: worst {worst:.1f} u")
    assert sum(s[0] == 1.0 for s in scores) >= 3 and sum(0.0 < s[0] < 1.0 for s in scores) >= 20
    assert CL.normalized_mutual_info([7, 7, 7], [1, 1, 1]) == 1.0 and CL.adjusted_rand([7, 7, 7], [1, 1, 1]) == 1.0
    assert CL.normalized_mutual_info([0, 0, 1, 1], [5, 5, 5, 5]) == 0.0
    assert CL.adjusted_rand(["a", "a", "b"], [3, 3, 9]) == 1.0                    # fp == fn == 0
    assert CL.normalized_mutual_info(torch.tensor([0, 1, 0, 1]), np.array([1, 0, 1, 0])) == 1.0


@pytest.mark.parametrize("name", sorted(RC.knn_cases()))
def test_total_order_gives_sklearns_knn_accuracy(name):
    x, y, k = RC.knn_cases()[name]
    assert RC.knn_margin_ok(x, y, k)
    assert RC.knn_accuracy(RC.sqdist_truth(x), y, k) == golden()["knn"][name]
    if name == "vote_tie":
        assert golden()["knn"][name] == 0.5 and (RC.knn_predict(RC.sqdist_truth(x), y, k) == 0).all()
    else:
        d2 = RC.sqdist_truth(x)
        assert ((d2 == 0).sum(axis=1) == 2).sum() == 2                            # the duplicated rows


# ------------------------------------------------------------------------------------------------ the binding and the refusals
def test_header_constants_and_symbols():
    from viscy_amd import _lib, ops

    assert (_lib.F64_TILE, _lib.F64_KC) == (64, 32) and ops.F64_TILE is _lib.F64_TILE and ops.F64_KC is _lib.F64_KC
    assert (_lib.PDIST_COSINE, _lib.PDIST_EUCLIDEAN, _lib.PDIST_SQEUCLIDEAN) == (0, 1, 2)
    assert {"vsx_row_sqnorm_f64", "vsx_pdist_f64", "vsx_eps_graph", "vsx_cc_round", "vsx_dbscan_finish"} <= set(_lib.exported_symbols())
    assert ops.eps_graph_words(1) == 1 and ops.eps_graph_words(64) == 1 and ops.eps_graph_words(65) == 2
    assert CL.MAX_GRAPH_BYTES == 16 << 30


def test_refusals_that_need_no_device(monkeypatch):
    x = RC.real_features(12, 5, 3)
    with pytest.raises(ValueError, match="cityblock"):
        CL.pairwise_distance_matrix(x, metric="cityblock")
    for device in ("cpu", None, "scipy"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CL.pairwise_distance_matrix(x, device=device)
    with pytest.raises(ValueError, match="Invalid device"):
        CL.pairwise_distance_matrix(x, device="tpu")
    with pytest.raises(ValueError, match="Invalid method. Choose 'nmi' or 'ari'."):
        CL.clustering_evaluation(x, np.arange(12), method="purity")
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        CL.knn_accuracy(x, np.arange(12), k=65)
    with pytest.raises(ValueError, match="eps"):
        CL.dbscan_clustering(x, eps=0.0)
    with pytest.raises(ValueError, match="min_samples"):
        CL.dbscan_clustering(x, min_samples=0)
    monkeypatch.setattr(CL, "MAX_GRAPH_BYTES", 95)
    with pytest.raises(ValueError, match="MAX_GRAPH_BYTES = 95"):
        CL.dbscan_clustering(x)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="above MAX_GRAPH_BYTES"):                # 400 000 rows: 20 GB of bits; nothing is allocated
        CL.dbscan_clustering(np.broadcast_to(np.zeros((1, 4), dtype=np.float32), (400000, 4)))
    if not torch.cuda.is_available():
        for fn in (lambda: CL.pairwise_distance_matrix(x), lambda: CL.dbscan_clustering(x), lambda: CL.knn_accuracy(x, np.arange(12), k=3),
                   lambda: CL.clustering_evaluation(x, np.arange(12))):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn()
