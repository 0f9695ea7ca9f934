"""CPU: the fixtures of the MMD tests are sound (the float64 restatement of tests/ref_mmd.py agrees with the reference's recorded
results within err_ref, every case keeps its null values 100 err_ref away from the observed one, so p-values compare for
equality), viscy_amd.mmd draws the reference's label matrix, refuses what it does not serve with ValueError before it looks for a
device, and the C-ABI of csrc/mmd.hip checks its arguments before any launch."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ref_mmd as RM
from tests.conftest import load_golden


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("mmd.pt")["cases"]


def test_the_golden_covers_the_case_table():
    assert sorted(golden()) == sorted(RM.CASES)
    for name in RM.CASES:
        g = golden()[name]
        assert g["null"].shape == (RM.CASES[name]["P"],) and g["null"].dtype == torch.float32
        assert ("labels" in g) == (name in RM.LABEL_CASES) and ("kernel" in g) == (name in RM.KERNEL_CASES)


@pytest.mark.parametrize("name", list(RM.CASES))
def test_restatement_agrees_with_the_reference_and_the_p_value_is_decided(name):
    c, g = RM.CASES[name], golden()[name]
    ours = RM.restatement(name, g["bandwidth"])
    err = max(abs(g["mmd2"] - ours[0]), float(np.abs(g["null"].numpy().astype(np.float64) - ours[1:]).max()))
    assert err <= g["err_ref"]                      # the recorded error is this restatement's
    assert g["err_ref"] < 5e-7                      # fp32 kernel values and fp32 sums of the reference: a few 1e-7
    gap = float(np.abs(ours[1:] - ours[0]).min())
    assert gap == pytest.approx(g["gap"], rel=1e-6) and gap >= 100 * g["err_ref"], (gap, g["err_ref"])
    assert float((np.sum(ours[1:] >= ours[0]) + 1) / (c["P"] + 1)) == g["p_value"]
    assert g["dist_err_f32"] == pytest.approx(RM.dist_err_f32(*RM.build(name)), rel=1e-3)


def test_case_table_probes_what_it_claims():
    c = RM.CASES
    assert (c["n70_m61_d33_p130"]["n"] + c["n70_m61_d33_p130"]["m"]) % 128 == 3 and c["n70_m61_d33_p130"]["d"] % 4 != 0
    assert c["n64_m64_d32_p64"]["n"] + c["n64_m64_d32_p64"]["m"] == 128
    assert c["n200_m157_d768_p257"]["P"] > 256 and c["n200_m157_d768_p257"]["d"] == 768
    assert 0.2 < golden()["n150_m150_d16_p200_null"]["p_value"] < 0.8
    assert c["n600_m500_d16_p40"]["n"] + c["n600_m500_d16_p40"]["m"] > RM.SUBSAMPLE
    # the offset case is the one that needs the centring: the uncentred fp32 Gram form is two orders of magnitude worse there
    X, Y = RM.build("n90_m100_d64_p100_offset10")
    pool = np.concatenate([X, Y])
    nrm = (pool * pool).sum(1, dtype=np.float32)
    raw = np.maximum(nrm[:, None] + nrm[None, :] - np.float32(2) * (pool @ pool.T), np.float32(0))
    d64 = RM.sqdist64(pool, pool)
    assert np.abs(raw - d64).max() > 30 * np.abs(RM.gram_sqdist_f32(pool) - d64).max()


@pytest.mark.parametrize("name", RM.LABEL_CASES)
def test_permutation_labels_equal_the_references(name):
    from viscy_amd.mmd import permutation_labels

    c, g = RM.CASES[name], golden()[name]
    z = permutation_labels(c["n"], c["m"], c["P"], c["pseed"])
    assert z.dtype == np.uint8 and z.shape == (c["P"] + 1, c["n"] + c["m"])
    assert np.array_equal(z, g["labels"].numpy())
    assert np.array_equal(z, RM.permutation_labels(c["n"], c["m"], c["P"], c["pseed"]))
    assert (z.sum(1) == c["n"]).all() and (z[0, : c["n"]] == 1).all()


def test_every_value_error_fires_before_a_device_is_looked_for():
    from viscy_amd import mmd

    rng = np.random.RandomState(0)
    X, Y = rng.randn(6, 3).astype(np.float32), rng.randn(5, 3).astype(np.float32)
    bad = X.copy()
    bad[2, 1] = np.nan
    inf = torch.from_numpy(Y.copy())
    inf[0, 0] = float("inf")
    for fn in (mmd.compute_mmd_unbiased, mmd.mmd_permutation_test):
        with pytest.raises(ValueError, match="at least two rows"):
            fn(X[:1], Y, bandwidth=1.0)
        with pytest.raises(ValueError, match="at least two rows"):
            fn(X, Y[:1], bandwidth=1.0)
        with pytest.raises(ValueError, match="bandwidth"):
            fn(X, Y, bandwidth=0.0)
        with pytest.raises(ValueError, match="bandwidth"):
            fn(X, Y, bandwidth=-1.0)
        with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
            fn(bad, Y, bandwidth=1.0)
        with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
            fn(X, inf, bandwidth=1.0)
        with pytest.raises(ValueError, match="differ in width"):
            fn(X, Y[:, :2], bandwidth=1.0)
    with pytest.raises(ValueError, match="n_permutations"):
        mmd.mmd_permutation_test(X, Y, n_permutations=0, bandwidth=1.0)
    with pytest.raises(ValueError, match="bandwidth"):
        mmd.gaussian_rbf_kernel(X, Y, 0.0)
    with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
        mmd.gaussian_rbf_kernel(bad, Y, 1.0)
    with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
        mmd.median_heuristic(bad, Y)
    with pytest.raises(ValueError, match="two pooled rows"):
        mmd.median_heuristic(X[:1], Y[:0])


def test_no_cpu_fallback(monkeypatch):
    from viscy_amd import mmd, ops

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # what a machine without a HIP device answers
    X, Y = np.zeros((4, 3), dtype=np.float32), np.ones((4, 3), dtype=np.float32)
    for call in (lambda: mmd.median_heuristic(X, Y), lambda: mmd.gaussian_rbf_kernel(X, Y, 1.0),
                 lambda: mmd.compute_mmd_unbiased(X, Y, 1.0), lambda: mmd.mmd_permutation_test(X, Y, 3, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.mmd_prepare(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.mmd_sums(torch.zeros(4, 3), torch.zeros(4), torch.zeros(1, 4, dtype=torch.uint8), 1.0)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """VSX_CHECK errors: nothing is launched, so this runs without a device (the pointers are host arrays no kernel ever sees)"""
    from viscy_amd import _lib

    l = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    tiles = lambda N: (N + 127) // 128  # noqa: E731
    # the workspace: one row of 2 (P + 1) doubles per workgroup; the split of the column tiles depends on N alone
    assert l.vsx_mmd_sums_ws_bytes(131, 130) == 2 * 2 * 2 * 131 * 8                 # 2 row tiles x 2 splits
    assert l.vsx_mmd_sums_ws_bytes(1100, 40) == 9 * 9 * 2 * 41 * 8                  # 9 x 9
    assert l.vsx_mmd_sums_ws_bytes(20000, 1000) == tiles(20000) * 4 * 2 * 1001 * 8  # 157 row tiles x 4 splits: 20 MB, not 1.6 GB
    assert l.vsx_mmd_sums_ws_bytes(4, 1) == 2 * 2 * 8
    for N, P in ((1, 4), (0, 4), (8, 0), ((1 << 24) + 1, 4), (8, (1 << 24) + 1)):
        assert l.vsx_mmd_sums_ws_bytes(N, P) == 0, (N, P)
    big = 1 << 40
    for args, msg in (((p, p, p, 1, 4, 3, 1.0, p, p, big, None), b"N=1 must be at least 2"),
                      ((p, p, p, 0, 4, 3, 1.0, p, p, big, None), b"N=0 must be in [1, 2^24]"),
                      ((p, p, p, 8, 0, 3, 1.0, p, p, big, None), b"d=0 must be in [1, 2^20]"),
                      ((p, p, p, 8, 4, 0, 1.0, p, p, big, None), b"P=0 must be in [1, 2^24]"),
                      ((p, p, p, 8, 4, 3, 0.0, p, p, big, None), b"bandwidth=0 must be positive"),
                      ((p, p, p, 8, 4, 3, -2.0, p, p, big, None), b"bandwidth=-2 must be positive"),
                      ((p, p, p, 8, 4, 3, float("nan"), p, p, big, None), b"must be positive"),
                      ((p, p, p, 8, 4, 3, 1e39, p, p, big, None), b"finite float"),
                      ((p, None, p, 8, 4, 3, 1.0, p, p, big, None), b"null argument"),
                      ((p, p, p, 8, 4, 3, 1.0, p + 4, p, big, None), b"8-byte aligned"),
                      ((p + 2, p, p, 8, 4, 3, 1.0, p, p, big, None), b"4-byte aligned"),
                      ((p, p, p, 8, 4, 3, 1.0, p, p, 63, None), b"vsx_mmd_sums_ws_bytes = 64 bytes (got 63)")):
        assert l.vsx_mmd_sums(*args) == 1 and msg in l.vsx_last_error(), (args[3:7], l.vsx_last_error())
    for args, msg in (((p, p, p, p, 0, 4, None), b"N=0"), ((p, p, p, p, 4, 0, None), b"d=0"), ((p, p, None, p, 4, 4, None), b"null argument"),
                      ((p, p + 1, p, p, 4, 4, None), b"4-byte aligned")):
        assert l.vsx_mmd_prepare(*args) == 1 and msg in l.vsx_last_error(), l.vsx_last_error()
    for args, msg in (((p, p, 8, 4, 0, 0, 0, 8, 1.0, 0, p, None), b"[0, 0) x [0, 8) is not a rectangle of 8 rows"),
                      ((p, p, 8, 4, 0, 9, 0, 8, 1.0, 0, p, None), b"is not a rectangle"),
                      ((p, p, 8, 4, 0, 8, -1, 8, 1.0, 0, p, None), b"is not a rectangle"),
                      ((p, p, 8, 4, 0, 8, 4, 3, 1.0, 0, p, None), b"is not a rectangle"),
                      ((p, p, 8, 4, 0, 8, 0, 8, 0.0, 0, p, None), b"bandwidth=0"),
                      ((p, p, 8, 4, 0, 8, 0, 8, 1.0, 0, None, None), b"null argument")):
        assert l.vsx_rbf_block(*args) == 1 and msg in l.vsx_last_error(), l.vsx_last_error()
    for args, msg in (((p, p, 1, 4, p, None), b"M=1 must be in [2, 65536]"), ((p, p, 65537, 4, p, None), b"M=65537"),
                      ((p, p, 4, 0, p, None), b"d=0"), ((p, None, 4, 4, p, None), b"null argument")):
        assert l.vsx_sqdist_upper(*args) == 1 and msg in l.vsx_last_error(), l.vsx_last_error()
