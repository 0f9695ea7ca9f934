"""GPU: viscy_amd.clustering and the kernels under it (csrc/clustering.hip on the float64 tile engine of csrc/f64_tile.h).

T = VSX_F64_TILE, KC = VSX_F64_KC.  Shapes: N in {1, 2, T - 1, T, T + 1, 2 T + 1} x d in {1, 3, KC - 1, KC, KC + 1, 4 KC + 3} and
one d = 768 case.

Distances.  Lattice features (integers, |v| <= 512: every dot is exact): the Euclidean output is array_equal to np.sqrt of the
exact integer d2, the squared one to d2 itself, the norms to the integer norms.  Real features with a zero row and duplicate rows:
squared Euclidean within 2 (d + 8) u (n_i + n_j) of the difference-form truth, cosine within 4 (d + 8) u of the long-double
truth (u = 2^-53; tests/ref_clustering.py); duplicate rows exactly 0 apart (Euclidean); out == out.T bit for bit; zero diagonal;
norms equal to the diagonal of the dots; block calls equal to slices of the whole matrix; a base 4 bytes off the 16-byte grid
(the scalar loader) gives the same bits.

Graph at N in {63, 64, 65, 129}: bits array_equal to d2 <= eps2 on lattices, pairs at exactly eps included; bits past N zero;
deg equal to the popcount.

DBSCAN against the golden sklearn labels (tests/golden/clustering.pt): lattices, the chain of 3 T + 5 points, the shared border
point, exactly min_samples neighbours, min_samples = 1, all noise, one cluster, blobs at d = 16 and 768; clustering_evaluation
for both methods (NMI within (R C + 16) u, ARI equal); knn_accuracy equal to sklearn's (vote tie to the smallest class, duplicate
rows).  Determinism: two runs equal, and a run after the workspace was filled with 0xFF bytes.  Refusals before any launch."""

import functools

import numpy as np
import pytest
import torch

from tests import ref_clustering as RC
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tile():
    from viscy_amd import ops

    return ops.F64_TILE, ops.F64_KC


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("clustering.pt")


@functools.lru_cache(maxsize=None)
def dbscan_cases():
    return RC.dbscan_cases(_tile()[0])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def off_grid(xd):
    """a copy of xd 4 bytes off the 16-byte grid"""
    flat = torch.empty(xd.numel() + 1, dtype=xd.dtype, device=DEV)
    view = flat[1:].view(xd.shape)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4
    return view


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def matrices(x):
    """-> (norms, {metric: (N, N) ndarray}) of the kernel"""
    from viscy_amd import ops

    xd = dev(x)
    norms = ops.row_sqnorm_f64(xd)
    return norms.cpu().numpy(), {m: ops.pdist_f64(xd, norms, m).cpu().numpy() for m in ("cosine", "euclidean", "sqeuclidean")}


def shapes():
    T, KC = 64, 32      # the header's values, asserted in test_constants; parametrize runs before the library is loaded
    return [(n, d) for n in (1, 2, T - 1, T, T + 1, 2 * T + 1) for d in (1, 3, KC - 1, KC, KC + 1, 4 * KC + 3)] + [(T + 1, 768)]


def test_constants():
    from viscy_amd import _lib

    assert _tile() == (_lib.F64_TILE, _lib.F64_KC) == (64, 32)


# ------------------------------------------------------------------------------------------------ distances
@pytest.mark.parametrize("n,d", shapes())
def test_lattice_distances_are_exact(n, d):
    x = RC.lattice_features(n, d, 1000 + n + d)
    d2 = RC.sqdist_truth(x)                                   # exact integers
    assert d2.max(initial=0.0) < 2.0 ** 53 and (d2 == np.rint(d2)).all()
    norms, got = matrices(x)
    assert same_bits(norms, RC.sqnorms(x))
    assert same_bits(got["sqeuclidean"], d2)
    assert same_bits(got["euclidean"], np.sqrt(d2))
    assert same_bits(got["cosine"], got["cosine"].T.copy()) and (np.diag(got["cosine"]) == 0.0).all()


@pytest.mark.parametrize("n,d", shapes())
def test_real_distances_within_the_bounds(n, d):
    from viscy_amd import ops

    x = RC.real_features(n, d, 2000 + n + d, zero_row=3, duplicates=((0, 1), (0, n - 1)))
    norms, got = matrices(x)
    off = RC.off_diagonal(n)
    err2 = np.abs(got["sqeuclidean"] - RC.sqdist_truth(x))
    errc = np.abs(got["cosine"] - RC.cosine_truth(x))
    bound2 = RC.sqdist_bound(x)
    print(f"N {n} d {d}: d2 error / bound {np.max(err2[off] / np.maximum(bound2[off], 1e-300), initial=0.0):.3f}, "
          f"cosine error {errc[off].max(initial=0.0) / RC.U:.1f} u of {RC.cosine_bound(x) / RC.U:.0f} u")
    assert (err2 <= bound2)[off].all()
    assert (errc[off] <= RC.cosine_bound(x)).all()
    if n > 3:
        assert (got["cosine"][3][np.arange(n) != 3] == 1.0).all()          # the zero row: F.normalize's rule
    for m, out in got.items():
        assert (np.diag(out) == 0.0).all(), m
        assert same_bits(out, out.T.copy()), m
    assert same_bits(got["euclidean"], np.sqrt(got["sqeuclidean"]))
    if n >= 2:
        assert got["euclidean"][0, 1] == 0.0 and got["euclidean"][0, n - 1] == 0.0 and got["sqeuclidean"][1, n - 1] == 0.0
        assert norms[0] == norms[1] == norms[n - 1]
    # the norms are the dots' diagonal: n_i + n_i - 2 dot_ii == 0 is what the duplicate rows show; and the scalar loader
    xo = off_grid(dev(x))
    no = ops.row_sqnorm_f64(xo)
    assert same_bits(no.cpu().numpy(), norms)
    assert same_bits(ops.pdist_f64(xo, no, "cosine").cpu().numpy(), got["cosine"])


def test_blocks_equal_slices():
    from viscy_amd import ops

    T, _ = _tile()
    n = 2 * T + 1
    x = RC.real_features(n, 35, 7, zero_row=5, duplicates=((1, 70),))
    xd = dev(x)
    norms = ops.row_sqnorm_f64(xd)
    for metric in ("cosine", "euclidean", "sqeuclidean"):
        whole = ops.pdist_f64(xd, norms, metric).cpu().numpy()
        for (r0, r1), (c0, c1) in (((0, n), (0, n)), ((1, T), (T - 1, n)), ((T, T + 1), (0, 3)), ((5, 2 * T), (5, 2 * T)),
                                   ((2 * T, n), (2 * T, n)), ((T + 3, n), (0, T + 3))):
            block = ops.pdist_f64(xd, norms, metric, rows=(r0, r1), cols=(c0, c1)).cpu().numpy()
            assert same_bits(block, np.ascontiguousarray(whole[r0:r1, c0:c1])), (metric, r0, r1, c0, c1)


@pytest.mark.parametrize("name", RC.DISTANCE_CASES)
def test_pairwise_distance_matrix_against_the_reference(name):
    from viscy_amd import clustering as CL

    x = RC.distance_case(name)
    off = RC.off_diagonal(len(x))
    for metric in ("cosine", "euclidean"):
        got = CL.pairwise_distance_matrix(x, metric=metric)
        want = golden()["dist"][name][metric].numpy()
        assert got.dtype == np.float64 and got.shape == want.shape and (np.diag(got) == 0.0).all()
        if metric == "cosine":
            assert (np.abs(got - want)[off] <= 2 * RC.cosine_bound(x)).all()      # either side is within one bound of the truth
        else:
            assert (np.abs(got ** 2 - want ** 2)[off] <= 2 * RC.sqdist_bound(x)[off] + 4 * RC.U * want[off] ** 2).all()
    assert same_bits(CL.pairwise_distance_matrix(torch.from_numpy(x).to(DEV), "euclidean", device="cuda"), got)


def test_pairwise_distance_matrix_in_row_blocks(monkeypatch):
    from viscy_amd import clustering as CL

    x = RC.real_features(150, 20, 5)
    whole = CL.pairwise_distance_matrix(x, "euclidean")
    monkeypatch.setattr(CL, "MAX_MATRIX_BYTES", 1024)
    monkeypatch.setattr(CL, "BLOCK_BYTES", 150 * 8 * 64)
    assert same_bits(CL.pairwise_distance_matrix(x, "euclidean"), whole)
    one = CL.pairwise_distance_matrix(x[:1], "cosine")
    assert one.shape == (1, 1) and one[0, 0] == 0.0


def test_ranks_on_the_device():
    from viscy_amd import clustering as CL

    dist = CL.pairwise_distance_matrix(RC.distance_case("real_20x3"), "euclidean")     # duplicate rows: ties
    for normalize in (False, True):
        want = RC.rank_nearest_neighbors(dist, normalize)
        got = CL.rank_nearest_neighbors(dev(dist), normalize)
        assert got.is_cuda and same_bits(got.cpu().numpy(), want)
        assert same_bits(CL.rank_nearest_neighbors(dist, normalize), want)


# ------------------------------------------------------------------------------------------------ the graph
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_graph_bits(n):
    from viscy_amd import ops

    x = RC.lattice_cloud(n, 3, 6, 40 + n)
    d2 = RC.sqdist_truth(x)
    xd = dev(x)
    norms = ops.row_sqnorm_f64(xd)
    for eps2 in (0.0, 1.0, 2.0, 4.0, 1e9):
        assert eps2 in (0.0, 1e9) or (d2 == eps2).sum() > 0            # pairs at exactly eps
        want_adj, want_deg = RC.graph_bits(d2, eps2)
        adj = torch.full((n, ops.eps_graph_words(n)), -1, dtype=torch.int64, device=DEV)
        deg = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        ops.eps_graph(xd, norms, eps2, adj, deg)
        got = adj.cpu().numpy().view(np.uint64)
        assert same_bits(got, want_adj), eps2
        assert same_bits(deg.cpu().numpy(), want_deg)
        if n % 64:
            assert (got[:, -1] >> np.uint64(n % 64) == 0).all()        # bits past N
        assert (np.array([bin(int(w)).count("1") for w in got.reshape(-1)]).reshape(got.shape).sum(axis=1) == want_deg).all()


# ------------------------------------------------------------------------------------------------ DBSCAN
DBSCAN_NAMES = ("lattice_2d", "lattice_3d", "lattice_2d_min1", "chain", "shared_border_4", "shared_border_5", "all_noise", "blobs_16",
                "blobs_768")


@pytest.mark.parametrize("name", DBSCAN_NAMES)
def test_dbscan_labels_are_sklearns(name):
    from viscy_amd import clustering as CL

    x, eps, min_samples = dbscan_cases()[name]
    want = golden()["dbscan"][name].numpy()
    got = CL.dbscan_clustering(x, eps=eps, min_samples=min_samples)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if name == "chain":
        assert (got == 0).all() and len(got) == 3 * _tile()[0] + 5
    if name == "shared_border_4":
        assert got[0] == 0 and set(got[1:5]) == {0} and set(got[5:]) == {1}
    if name == "all_noise":
        assert (got == -1).all()
    assert np.array_equal(CL.dbscan_clustering(torch.from_numpy(x).to(DEV), eps, min_samples), want)


def test_dbscan_is_deterministic_and_ignores_the_workspace():
    from viscy_amd import clustering as CL

    x, eps, min_samples = dbscan_cases()["lattice_3d"]
    first = CL.dbscan_clustering(x, eps, min_samples)
    assert np.array_equal(CL.dbscan_clustering(x, eps, min_samples), first)
    ws = CL.graph_workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    assert ws.numel() >= len(x) * 3 * 8
    ws.fill_(0xFF)
    assert np.array_equal(CL.dbscan_clustering(x, eps, min_samples), first)
    ws.fill_(0xFF)
    x2, eps2, ms2 = dbscan_cases()["chain"]
    assert (CL.dbscan_clustering(x2, eps2, ms2) == 0).all()


@pytest.mark.parametrize("d", [16, 768])
def test_clustering_evaluation(d):
    from viscy_amd import clustering as CL

    x, _, noisy = RC.blob_case(d)[1]
    want = golden()["eval"]["blobs_%d" % d]
    nmi, ari = CL.clustering_evaluation(x, noisy, method="nmi"), CL.clustering_evaluation(x, noisy, method="ari")
    assert isinstance(nmi, float) and isinstance(ari, float)
    clusters = golden()["dbscan"]["blobs_%d" % d].numpy()
    assert abs(nmi - want["nmi"]) <= RC.nmi_bound(len(np.unique(noisy)), len(np.unique(clusters)))
    assert ari == want["ari"]


@pytest.mark.parametrize("name", ["vote_tie", "blobs_16", "blobs_768"])
def test_knn_accuracy(name):
    from viscy_amd import clustering as CL

    x, y, k = RC.knn_cases()[name]
    got = CL.knn_accuracy(x, y, k=k)
    assert isinstance(got, float) and got == golden()["knn"][name]
    assert got == RC.knn_accuracy(RC.sqdist_truth(x), y, k)
    if name == "vote_tie":
        assert got == 0.5
    assert CL.knn_accuracy(torch.from_numpy(x).to(DEV), [str(v) for v in y], k=k) == got      # class names instead of numbers


def test_knn_accuracy_in_row_blocks(monkeypatch):
    from viscy_amd import clustering as CL

    x, y, k = RC.knn_cases()["blobs_16"]
    monkeypatch.setattr(CL, "BLOCK_BYTES", 1)
    assert CL.knn_accuracy(x, y, k=k) == golden()["knn"]["blobs_16"]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(monkeypatch):
    from viscy_amd import _lib, ops
    from viscy_amd import clustering as CL

    launched = []
    real = _lib.lib
    x = RC.real_features(12, 5, 3)

    class Counting:
        """every library function called from here on is recorded"""

        def __getattr__(self, name):
            launched.append(name)
            return getattr(real(), name)

    monkeypatch.setattr(ops, "lib", lambda: Counting())
    cpu = torch.from_numpy(x)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.row_sqnorm_f64(cpu)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.pdist_f64(cpu, torch.zeros(12, dtype=torch.float64), "cosine")
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.eps_graph(cpu, torch.zeros(12, dtype=torch.float64), 1.0)
    bad = x.copy()
    bad[3, 2] = np.nan
    for fn in (lambda: CL.pairwise_distance_matrix(bad), lambda: CL.dbscan_clustering(bad), lambda: CL.knn_accuracy(bad, np.arange(12) % 2, k=3),
               lambda: CL.clustering_evaluation(dev(bad), np.arange(12) % 2)):
        with pytest.raises(ValueError, match="NaN or infinity"):
            fn()
    with pytest.raises(ValueError, match="cityblock"):
        CL.pairwise_distance_matrix(x, metric="cityblock")
    for device in ("cpu", None, "scipy"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CL.pairwise_distance_matrix(x, device=device)
    with pytest.raises(ValueError, match="Invalid device"):
        CL.pairwise_distance_matrix(x, device="tpu")
    with pytest.raises(ValueError, match="sqeuclid"):
        ops.pdist_f64(dev(x), torch.zeros(12, dtype=torch.float64, device=DEV), "sqeuclid")
    with pytest.raises(ValueError, match="n_neighbors = 13"):
        CL.knn_accuracy(x, np.arange(12) % 2, k=13)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        CL.knn_accuracy(x, np.arange(12) % 2, k=0)
    with pytest.raises(ValueError, match="Invalid method. Choose 'nmi' or 'ari'."):
        CL.clustering_evaluation(x, np.arange(12) % 2, method="purity")
    monkeypatch.setattr(CL, "MAX_GRAPH_BYTES", 95)
    with pytest.raises(ValueError, match="MAX_GRAPH_BYTES = 95"):
        CL.dbscan_clustering(x)                  # 12 rows x 1 word x 8 bytes = 96
    assert launched == []
    # the library's own refusals: a status, a message, no launch
    l = real()
    xd, nd, out = dev(x), torch.zeros(12, dtype=torch.float64, device=DEV), torch.zeros((12, 12), dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert l.vsx_pdist_f64(xd.data_ptr(), nd.data_ptr(), 12, 5, 3, 0, 12, 0, 12, out.data_ptr(), 12, st) != 0 and b"metric" in l.vsx_last_error()
    assert l.vsx_pdist_f64(xd.data_ptr(), nd.data_ptr(), 12, 5, 0, 0, 13, 0, 12, out.data_ptr(), 12, st) != 0 and b"block" in l.vsx_last_error()
    assert l.vsx_pdist_f64(xd.data_ptr(), nd.data_ptr(), 12, 5, 0, 0, 12, 0, 12, out.data_ptr(), 11, st) != 0 and b"ld=11" in l.vsx_last_error()
    assert l.vsx_pdist_f64(xd.data_ptr(), nd.data_ptr() + 4, 12, 5, 0, 0, 12, 0, 12, out.data_ptr(), 12, st) != 0
    assert l.vsx_row_sqnorm_f64(xd.data_ptr(), 0, 5, nd.data_ptr(), st) != 0 and l.vsx_row_sqnorm_f64(None, 12, 5, nd.data_ptr(), st) != 0
    assert l.vsx_eps_graph(xd.data_ptr(), nd.data_ptr(), 12, 5, float("nan"), out.data_ptr(), out.data_ptr(), st) != 0
    assert l.vsx_cc_round(None, out.data_ptr(), out.data_ptr(), 12, out.data_ptr(), st) != 0
    assert l.vsx_dbscan_finish(out.data_ptr(), out.data_ptr(), out.data_ptr(), None, 12, out.data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert (out == 0).all() and (nd == 0).all()
