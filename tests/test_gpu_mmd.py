"""GPU: viscy_amd.mmd and the kernels of csrc/mmd.hip under it.

Accuracy (tests/golden/mmd.pt, tests/ref_mmd.py).  With the reference's bandwidth, mmd2 and every null value are within
4 err_ref of the float64 restatement (err_ref: the reference's own distance from it, 2e-7 .. 3e-7; the device rounds the distance
as well as the kernel value) and the p-value EQUALS the reference's (every case keeps its null values 100 err_ref away from the
observed one).  The median heuristic is within 4 dist_err_f32 of the reference's (the median is 1-Lipschitz in the sup norm of the
distances; dist_err_f32 is the error of a float32 numpy emulation of the centred Gram form).  gaussian_rbf_kernel is within
relative 4 exponent_err_f32 + 2^-23 of the reference's matrix.

Exact properties of the tile, through the ops wrappers: symmetry of the kernel bit for bit, a zero diagonal, sums of one- and
two-hot label vectors against rbf_block bit for bit, label rows permuted = output rows permuted, the same row 0 for any P, two
runs bit-identical, a run on poisoned allocations equal to a clean one.  The sums of arbitrary label vectors are compared with
float64 sums of the materialised device kernel within the worst-case bound of a 128-term fp32 accumulation."""

import functools

import numpy as np
import pytest
import torch

from tests import ref_exact_tile as XT
from tests import ref_mmd as RM
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("mmd.pt")["cases"]


@functools.lru_cache(maxsize=None)
def device_run(name):
    """mmd_permutation_test on the case with the reference's bandwidth, once"""
    from viscy_amd.mmd import mmd_permutation_test

    c = RM.CASES[name]
    X, Y = RM.build(name)
    obs, p, null = mmd_permutation_test(X, Y, n_permutations=c["P"], bandwidth=golden()[name]["bandwidth"], seed=c["pseed"])
    null.setflags(write=False)
    return obs, p, null


@pytest.mark.parametrize("name", list(RM.CASES))
def test_permutation_test_against_the_restatement_and_the_reference(name):
    c, g = RM.CASES[name], golden()[name]
    obs, p, null = device_run(name)
    ours = RM.restatement(name, g["bandwidth"])
    assert isinstance(obs, float) and isinstance(p, float) and null.dtype == np.float64 and null.shape == (c["P"],)
    err = max(abs(obs - ours[0]), float(np.abs(null - ours[1:]).max()))
    print(f"\n{name}: max |device - float64| {err:.3e}  bound 4 err_ref {4 * g['err_ref']:.3e}  (err_ref {g['err_ref']:.3e})  p {p:.6f}")
    assert err <= 4 * g["err_ref"]
    assert p == g["p_value"]
    assert abs(obs - g["mmd2"]) <= 5 * g["err_ref"]  # against the reference itself: its own err_ref on top


@pytest.mark.parametrize("name", list(RM.CASES))
def test_median_heuristic_against_the_reference(name):
    from viscy_amd.mmd import median_heuristic

    g = golden()[name]
    X, Y = RM.build(name)
    bw = median_heuristic(X, Y)
    print(f"\n{name}: |median - reference| {abs(bw - g['bandwidth']):.3e}  bound 4 dist_err_f32 {4 * g['dist_err_f32']:.3e}")
    assert isinstance(bw, float)
    assert abs(bw - g["bandwidth"]) <= 4 * g["dist_err_f32"]
    assert median_heuristic(torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(Y.copy()), subsample=RM.SUBSAMPLE) == bw  # tensors, either place


@pytest.mark.parametrize("name", list(RM.CASES))
def test_compute_mmd_unbiased_is_row_zero_and_symmetric(name):
    from viscy_amd.mmd import compute_mmd_unbiased

    g = golden()[name]
    X, Y = RM.build(name)
    obs = device_run(name)[0]
    v = compute_mmd_unbiased(X, Y, bandwidth=g["bandwidth"])
    assert isinstance(v, float) and v == obs                                      # bit for bit
    assert compute_mmd_unbiased(torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(Y.copy()).to(DEV), g["bandwidth"]) == obs
    assert abs(compute_mmd_unbiased(Y, X, bandwidth=g["bandwidth"]) - obs) <= 4 * g["err_ref"]


def test_default_bandwidth_is_the_median_heuristic():
    from viscy_amd.mmd import compute_mmd_unbiased, median_heuristic, mmd_permutation_test

    X, Y = RM.build("n20_m23_d5_p50")
    bw = median_heuristic(X, Y)
    assert compute_mmd_unbiased(X, Y) == compute_mmd_unbiased(X, Y, bandwidth=bw)
    a, b = mmd_permutation_test(X, Y, n_permutations=7), mmd_permutation_test(X, Y, n_permutations=7, bandwidth=bw, seed=42)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", RM.KERNEL_CASES)
def test_gaussian_rbf_kernel_against_the_reference(name):
    from viscy_amd.mmd import gaussian_rbf_kernel

    g = golden()[name]
    X, Y = RM.build(name)
    K = gaussian_rbf_kernel(X, Y, g["bandwidth"])
    ref = g["kernel"].numpy()
    assert isinstance(K, np.ndarray) and K.dtype == np.float32 and K.shape == ref.shape
    rel = float((np.abs(K.astype(np.float64) - ref) / ref).max())
    tol = 4 * g["exponent_err_f32"] + 2.0 ** -23
    print(f"\n{name}: max relative error {rel:.3e}  bound {tol:.3e}")
    assert rel <= tol


# ------------------------------------------------------------------------------------------------ exact properties of the tile
# N % 16 != 0, d % 4 == 0: byte label loads;  N % 16 == 0: 16-byte label loads;  25 column tiles in 13 splits of 2, the last of 1
# (tests/ref_exact_tile.mmd_plan): real kernel values on the accumulation over tiles, which the 0 / 1 values of
# tests/test_gpu_tile_exact.py cannot tell from values with a wrong exponent of the same class
POOLS = ("case357", "n272_d20", "n3075_d12")


@functools.lru_cache(maxsize=None)
def _pool(kind):
    """-> (xc, norms, bandwidth, K with a zero diagonal (device), N)"""
    from viscy_amd import ops

    if kind == "case357":
        x, bw = np.concatenate(RM.build("n200_m157_d768_p257")), golden()["n200_m157_d768_p257"]["bandwidth"]
    elif kind == "n272_d20":
        x, bw = np.random.RandomState(7).randn(272, 20).astype(np.float32), 18.0
    else:   # squared distances of unit normal rows: mean 2 d = 24, the median a little below
        x, bw = np.random.RandomState(11).randn(3075, 12).astype(np.float32), 23.0
    xc, norms, mean = ops.mmd_prepare(torch.from_numpy(x).to(DEV))
    N = len(x)
    assert np.abs(mean.cpu().numpy() - x.astype(np.float64).mean(0)).max() <= 2.0 ** -23 * np.abs(x).max()
    assert torch.equal(xc, torch.from_numpy(x).to(DEV) - mean)
    return xc, norms, bw, ops.rbf_block(xc, norms, (0, N), (0, N), bw, True), N


def _pairs(N):
    """(i, j) for the two-hot label vectors: tile corners and, where mmd_plan(N) gives a workgroup two or more column tiles, pairs
    in the second tile of a split, in two different splits, in the short last split and in the tail tile (row i meets column j
    and row j column i)"""
    pairs = [(0, 127), (127, 128), (0, N - 1), (N - 2, N - 1), (5, 5 + 128)]
    tiles, splits, tps, last = XT.mmd_plan(N)
    if tps >= 2:
        T, mid = XT.T, (splits // 2) * tps
        pairs += [(7, (mid + 1) * T + 9),                      # the second tile of a split; the rows' own split is the first
                  (mid * T + 3, (mid + 1) * T + 64),           # the first and the second tile of one split
                  ((tps + 1) * T + 1, (mid + tps + 1) * T + 5),  # second tiles of two different splits
                  (200, (splits - 1) * tps * T + (N - 1 - (splits - 1) * tps * T) // 2),   # the last split
                  ((mid + 1) * T + 2, N - 1 - (N - 1) % T)]    # the first row of the tail tile
    return pairs


@pytest.mark.parametrize("kind", POOLS)
def test_kernel_tile_is_symmetric_with_a_zero_diagonal(kind):
    from viscy_amd import ops

    xc, norms, bw, K, N = _pool(kind)
    assert torch.equal(K, K.t())
    assert (torch.diagonal(K) == 0.0).all()
    kept = ops.rbf_block(xc, norms, (0, N), (0, N), bw, False)
    off = ~torch.eye(N, dtype=torch.bool, device=DEV)
    assert torch.equal(kept[off], K[off]) and (torch.diagonal(kept) > 0.999).all()
    # a rectangle that starts inside a tile holds the same values
    sub = ops.rbf_block(xc, norms, (3, 131), (126, N), bw, True)
    assert torch.equal(sub, K[3:131, 126:N])
    x64 = xc.double().cpu().numpy()
    ref = np.exp(-RM.sqdist64(x64, x64) / (2.0 * bw))
    np.fill_diagonal(ref, 0.0)
    # worst case of the exponent: d + 4 fp32 roundings relative to n_i + n_j (dot, sum, difference, division), then expf's ulp
    tol = (xc.shape[1] + 4) * 2.0 ** -24 * 2.0 * float(norms.max()) / (2.0 * bw) + 2.0 ** -22
    assert np.abs(K.cpu().numpy() - ref).max() <= tol


@pytest.mark.parametrize("kind", POOLS)
def test_one_and_two_hot_label_vectors_give_kernel_entries_bit_for_bit(kind):
    from viscy_amd import ops

    xc, norms, bw, K, N = _pool(kind)
    pairs = _pairs(N)
    z = torch.zeros((2 * len(pairs), N), dtype=torch.uint8)
    for q, (i, j) in enumerate(pairs):
        z[2 * q, i] = 1
        z[2 * q + 1, i] = z[2 * q + 1, j] = 1
    s = ops.mmd_sums(xc, norms, z.to(DEV), bw).cpu()
    T = float(K.double().sum())
    for q, (i, j) in enumerate(pairs):
        assert s[2 * q, 0] == 0.0                                   # quad of a one-hot vector: the zero diagonal
        assert float(s[2 * q + 1, 0]) == 2.0 * float(K[i, j])          # k_ij + k_ji, exact in float64
        assert float(s[2 * q, 2]) == pytest.approx(float(K[i].double().sum()), rel=2.0 ** -15)   # sum_XY of a one-hot vector: row sum
        assert float(s[2 * q, 1]) == pytest.approx(T - 2 * float(K[i].double().sum()), rel=2.0 ** -15)


@pytest.mark.parametrize("kind", POOLS)
def test_sums_against_float64_sums_of_the_device_kernel(kind):
    """the kernel values are those of rbf_block; the second product accumulates 128 non-negative terms per column tile in fp32
    (worst case 128 * 2^-24 relative), everything after that is float64: every sum is within 4 * 2^-17 T of the float64 one"""
    from viscy_amd import ops

    xc, norms, bw, K, N = _pool(kind)
    z = RM.permutation_labels(N // 2, N - N // 2, 300, 5)
    s = ops.mmd_sums(xc, norms, torch.from_numpy(z).to(DEV), bw).cpu().numpy()
    ref = RM.sums(K.double().cpu().numpy(), z)
    T = ref[0].sum() + ref[0, 2]
    err = float(np.abs(s - ref).max())
    print(f"\n{kind}: max |sums - float64 sums of the device kernel| / T = {err / T:.3e}  bound {2.0 ** -15:.3e}")
    assert err <= 2.0 ** -15 * T


@pytest.mark.parametrize("kind", POOLS)
def test_label_rows_are_independent_and_runs_repeat(kind):
    from viscy_amd import debug, ops

    xc, norms, bw, _, N = _pool(kind)
    z = torch.from_numpy(RM.permutation_labels(N // 3, N - N // 3, 256, 9)).to(DEV)   # 257 rows
    s = ops.mmd_sums(xc, norms, z, bw)
    assert torch.equal(ops.mmd_sums(xc, norms, z, bw), s)                        # two runs
    with debug.poison_empty():
        assert torch.equal(ops.mmd_sums(xc, norms, z, bw), s)                    # the call initialises what it reads
    perm = torch.from_numpy(np.random.RandomState(3).permutation(257)).to(DEV)
    assert torch.equal(ops.mmd_sums(xc, norms, z[perm].contiguous(), bw), s[perm])
    assert torch.equal(ops.mmd_sums(xc, norms, z[:1].contiguous(), bw), s[:1])   # P = 1 and P = 257: the same row 0
    assert torch.equal(ops.mmd_sums(xc, norms, z[128:130].contiguous(), bw), s[128:130])


def test_public_functions_repeat_and_survive_poisoned_allocations():
    from viscy_amd import debug
    from viscy_amd.mmd import gaussian_rbf_kernel, median_heuristic, mmd_permutation_test

    name = "n70_m61_d33_p130"
    c, g = RM.CASES[name], golden()[name]
    X, Y = RM.build(name)
    obs, p, null = device_run(name)
    bw = median_heuristic(X, Y)
    K = gaussian_rbf_kernel(X, Y, g["bandwidth"])
    with debug.poison_empty():
        again = mmd_permutation_test(X, Y, n_permutations=c["P"], bandwidth=g["bandwidth"], seed=c["pseed"])
        assert again[0] == obs and again[1] == p and np.array_equal(again[2], null)
        assert median_heuristic(X, Y) == bw
        assert np.array_equal(gaussian_rbf_kernel(X, Y, g["bandwidth"]), K)


def test_sqdist_upper_is_the_upper_triangle_of_the_tile():
    from viscy_amd import ops

    xc, norms, _, _, N = _pool("n272_d20")
    up = ops.sqdist_upper(xc, norms)[0].cpu().numpy()
    i, j = np.triu_indices(N, 1)
    x64 = xc.double().cpu().numpy()
    ref = RM.sqdist64(x64, x64)[i, j]
    assert up.shape == (N * (N - 1) // 2,)
    assert np.abs(up - ref).max() <= 4 * np.abs(RM.gram_sqdist_f32(x64.astype(np.float32)).astype(np.float64)[i, j] - ref).max()


def test_squared_distances_hold_the_classifier_heads_dots_bit_for_bit():
    """f32_tile.h's one summation order for the third user: with zero norms sqdist_upper stores max(-2 dot, 0) (the doubling is
    exact), and the linear head without a bias stores the plain dot of the same two rows.  154 rows: two row tiles, the second
    partial; d = 36: one full chunk and one of 4 features.  pool = [x; -x] makes half of the dots negative (50.3 % in float64,
    the smallest |dot| 1.8e-3, far above fp32 error), so the clamp leaves half of the comparison non-trivial"""
    from viscy_amd import ops

    x = torch.randn(77, 36, generator=torch.Generator().manual_seed(0))
    pool = torch.cat([x, -x]).to(DEV)
    Z = ops.cls_logits(pool, pool)
    D = ops.sqdist_upper(pool, torch.zeros(154, device=DEV))[0]
    i, j = torch.triu_indices(154, 154, 1, device=DEV)
    assert D.shape == (11781,)
    assert torch.equal(D, torch.clamp_min(-2.0 * Z[i, j], 0.0))
    assert int((D != 0).sum()) >= 0.45 * 11781


def test_ops_refuse_what_they_do_not_serve():
    from viscy_amd import ops

    xc, norms, bw, _, N = _pool("n272_d20")
    with pytest.raises(TypeError, match="uint8"):
        ops.mmd_sums(xc, norms, torch.zeros((2, N), dtype=torch.int32, device=DEV), bw)
    with pytest.raises(TypeError, match="uint8"):
        ops.mmd_sums(xc, norms, torch.zeros((2, N + 1), dtype=torch.uint8, device=DEV), bw)
    with pytest.raises(RuntimeError, match="bandwidth"):
        ops.mmd_sums(xc, norms, torch.zeros((2, N), dtype=torch.uint8, device=DEV), 0.0)
    with pytest.raises(RuntimeError, match="rectangle"):
        ops.rbf_block(xc, norms, (0, N + 1), (0, N), bw, True)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.mmd_sums(xc.cpu(), norms, torch.zeros((2, N), dtype=torch.uint8, device=DEV), bw)
