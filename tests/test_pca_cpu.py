"""CPU: the fixtures of the PCA tests are sound (the float64 restatement of tests/ref_pca.py agrees with the reference's recorded
results within err_ref, err_ref is a few 1e-6, every compared component keeps a 1.2 x eigenvalue gap to both neighbours), the pure
host function of viscy_amd.reduce reproduces the restatement to float64 round-off from numpy's moments and Gram, viscy_amd.reduce
refuses what it does not serve before it looks for a device, and the C-ABI of csrc/pca.hip checks its arguments before any launch
and sizes its workspaces by the formulas restated in tests/ref_pca.py."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ref_pca as RP
from tests.conftest import load_golden

KEY = {True: "norm", False: "raw"}
CASE_MODES = [(name, nm) for name in RP.CASES for nm in RP.NORMALIZE]


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("pca.pt")["cases"]


def test_the_golden_covers_the_case_table():
    assert sorted(golden()) == sorted(RP.CASES)
    for name, c in RP.CASES.items():
        g = golden()[name]
        assert g["scaler_mean"].shape == (c["d"],) and g["scaler_mean"].dtype == torch.float64
        for nm in RP.NORMALIZE:
            e = g[KEY[nm]]
            k = e["n_components"]
            assert e["pc_features"].dtype == torch.float32 and e["pc_features"].shape == (c["N"], min(k, 16))
            assert e["components"].shape == (k, c["d"]) and e["explained_variance"].shape == (k,) and e["ratio"].shape == (k,)
            assert len(e["err_ref"]) == 3 and len(e["gram_err_f32"]) == 3


def test_case_table_probes_what_it_claims():
    c = RP.CASES
    assert {(v["N"], v["d"], v["k"]) for v in c.values()} >= {(2, 4, 1), (33, 33, None), (129, 128, 8), (300, 132, 8), (257, 260, 8),
                                                              (1300, 768, 8), (1000, 64, None), (600, 96, 0.9)}
    assert RP.gram_plan(1300, 768)[:3] == (6, 21, 3) and RP.gram_plan(257, 260)[:2] == (3, 6)
    r = RP.R132
    assert [RP.gram_plan(n, 132)[2:] for n in (r - 1, r, r + 1)] == [(1, r), (1, r), (2, r)] and r == 512
    assert c["n511_d132"]["N"] == r - 1 and c["n513_d132"]["N"] == r + 1 and c["n127_d132"]["N"] == RP.R - 1 and c["n129_d132"]["N"] == RP.R + 1
    assert c["n100_d132_wide"]["N"] < c["n100_d132_wide"]["d"]
    x = RP.build("n300_d132_const")
    assert (x[:, 5] == np.float32(3.25)).all() and RP.restatement("n300_d132_const")["scale"][5] == 1.0
    # the offset is what makes the centring matter: most columns sit several spreads away from the origin
    x = RP.build("n1300_d768_k8")
    assert np.median(np.abs(x.mean(0)) / x.std(0)) > 10


@pytest.mark.parametrize("name,normalize", CASE_MODES)
def test_restatement_agrees_with_the_reference_and_components_are_conditioned(name, normalize):
    c, e = RP.CASES[name], golden()[name][KEY[normalize]]
    ours = RP.restatement(name, normalize)
    idx = RP.compared(name, normalize)
    # a condition on the fixtures, not a tolerance: the planted components of every case with d >= 8 are compared
    lead = min(RP.PLANTED, c["N"] - 1, ours["n_components"])
    assert idx == list(range(lead if c["d"] >= 8 else 1)), (idx, ours["all_variance"][:10])
    assert all(RP.gaps_ok(ours["all_variance"], i) for i in range(min(RP.PLANTED, c["N"] - 1, c["d"])))
    assert ours["n_components"] == e["n_components"]
    res = dict(explained_variance=e["explained_variance"].numpy(), ratio=e["ratio"].numpy(), components=e["components"].numpy(),
               Z=e["pc_features"].numpy())
    err = RP.errors(res, ours, idx)
    assert err == pytest.approx(e["err_ref"], rel=1e-6, abs=1e-18)      # the recorded error is this restatement's
    assert e["err_ref"][0] <= 2e-6 and e["err_ref"][2] <= 2e-6 and e["err_ref"][1] <= 5e-7
    assert RP.signs_agree(res["components"], ours, RP.decided(name, normalize))
    # the flip is decided on every compared component but for two standardised rows (all entries of one magnitude)
    assert RP.decided(name, normalize) == ([] if (name == "n2_d4_k1" and normalize) else idx)
    assert RP.gram_err_f32(name, normalize) == pytest.approx(e["gram_err_f32"], rel=1e-6, abs=1e-18)


def test_scaler_statistics_agree_with_the_reference():
    for name in RP.CASES:
        g, r = golden()[name], RP.restatement(name, True)
        np.testing.assert_allclose(r["mean"], g["scaler_mean"].numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r["var"], g["scaler_var"].numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(r["scale"], g["scaler_scale"].numpy(), rtol=1e-9)


# ------------------------------------------------------------------------------------------------ the pure host function
@pytest.mark.parametrize("name,normalize", CASE_MODES)
def test_host_function_reproduces_the_restatement(name, normalize):
    from viscy_amd.reduce import pca_from_moments

    c, r = RP.CASES[name], RP.restatement(name, normalize)
    fit = pca_from_moments(c["N"], r["mean"], r["m2"], r["gram"], c["k"], normalize)
    assert fit.n_components_ == r["n_components"] and fit.n_samples == c["N"]
    top = r["all_variance"][0]
    for got, want in ((fit.explained_variance_, r["explained_variance"]), (fit.explained_variance_ratio_ * top, r["ratio"] * top),
                      (fit.singular_values_ ** 2 / (c["N"] - 1), r["singular_values"] ** 2 / (c["N"] - 1))):
        assert got.dtype == np.float64 and got.shape == (r["n_components"],)
        assert np.abs(got - want).max() <= 64 * c["d"] * 2.0 ** -52 * top
    assert abs(fit.noise_variance_ - r["noise_variance"]) <= 64 * c["d"] * 2.0 ** -52 * top
    idx = RP.compared(name, normalize)
    err = RP.errors(dict(explained_variance=fit.explained_variance_, ratio=fit.explained_variance_ratio_, components=fit.components_,
                         Z=r["Z"]), r, idx)
    assert err[1] <= 1e-24                                   # the same eigenvectors: angles of float64 round-off
    assert RP.signs_agree(fit.components_, r, idx)           # the flip, the undecided case included: the same float64 entries decide
    for i in range(fit.n_components_):
        assert fit.components_[i, np.argmax(np.abs(fit.components_[i]))] > 0.0
    assert np.abs(fit.components_ @ fit.components_.T - np.eye(fit.n_components_)).max() <= 1e-12
    np.testing.assert_array_equal(fit.scale, r["scale"])
    np.testing.assert_array_equal(fit.var, r["var"])
    np.testing.assert_array_equal(fit.mean_, np.zeros(c["d"]) if normalize else r["mean"])
    w = fit.projection_weights()
    assert w.dtype == np.float32 and w.shape == (fit.n_components_, c["d"])
    np.testing.assert_array_equal(w, (fit.components_ / r["scale"][None, :]).astype(np.float32))


def test_host_function_rules():
    from viscy_amd.reduce import pca_from_moments, scale_from_moments

    r = RP.restatement("n600_d96_f09", True)
    n, d = 600, 96
    args = (n, r["mean"], r["m2"], r["gram"])
    assert pca_from_moments(*args, None).n_components_ == 96
    assert pca_from_moments(*args, 7).n_components_ == 7 and pca_from_moments(*args, np.int64(7)).components_.shape == (7, d)
    ratio = r["all_variance"] / r["all_variance"].sum()
    for frac in (0.5, 0.9, 0.99, 0.999999):
        want = int(np.searchsorted(np.cumsum(ratio), frac, side="right")) + 1
        assert pca_from_moments(*args, frac).n_components_ == want
    assert pca_from_moments(*args, 96).noise_variance_ == 0.0
    assert pca_from_moments(*args, 5).noise_variance_ == pytest.approx(r["all_variance"][5:].mean(), rel=1e-12)
    wide = RP.restatement("n100_d132_wide", False)
    fit = pca_from_moments(100, wide["mean"], wide["m2"], wide["gram"], None, False)
    assert fit.n_components_ == 100 and fit.noise_variance_ == 0.0 and (fit.explained_variance_ >= 0.0).all()
    # clipping: a Gram with a negative eigenvalue (not a Gram at all) gives variances >= 0 and singular values without NaN
    g = np.diag([4.0, 1.0, -1e-9])
    fit = pca_from_moments(5, np.zeros(3), np.array([4.0, 1.0, 1.0]), g, None, False)
    np.testing.assert_array_equal(fit.explained_variance_, [1.0, 0.25, 0.0])
    assert np.isfinite(fit.singular_values_).all() and fit.singular_values_[2] == 0.0
    # the flip: the entry of largest magnitude is positive
    g = np.array([[2.0, -1.9], [-1.9, 2.0]])
    fit = pca_from_moments(3, np.zeros(2), np.array([2.0, 2.0]), g, None, False)
    assert fit.components_[0, np.argmax(np.abs(fit.components_[0]))] > 0 and fit.components_[0, 0] * fit.components_[0, 1] < 0
    # the constant-column rule is sklearn's: variance within n eps var + (n mean eps)^2
    var, scale = scale_from_moments(1000, np.array([1e8, 1.0, 0.0]), np.array([1e-9, 1e-9, 0.0]))
    assert scale[0] == 1.0 and scale[1] == np.sqrt(1e-12) and scale[2] == 1.0 and var[0] == 1e-12
    for bad in (0, -1, 97, 1.0, 1.5, 0.0, True):
        with pytest.raises(ValueError, match="n_components"):
            pca_from_moments(*args, bad)
    with pytest.raises(NotImplementedError, match="mle"):
        pca_from_moments(*args, "mle")
    with pytest.raises(ValueError, match="n_components"):
        pca_from_moments(*args, "arpack")


# ------------------------------------------------------------------------------------------------ errors before a device
def test_every_refusal_fires_before_a_device_is_looked_for(monkeypatch):
    from viscy_amd import reduce

    def no_device(*a, **k):
        raise AssertionError("a device was looked for")

    monkeypatch.setattr(reduce, "device_of", no_device)
    rng = np.random.RandomState(0)
    X = rng.randn(6, 3).astype(np.float32)
    bad = X.copy()
    bad[2, 1] = np.nan
    inf = torch.from_numpy(X.copy())
    inf[0, 0] = float("inf")
    for call in (lambda a, **k: reduce.compute_pca(a, **k), lambda a, **k: reduce.PCA(**k).fit(a), lambda a, **k: reduce.PCA(**k).fit_transform(a)):
        with pytest.raises(ValueError, match="matrix"):
            call(X[0])
        with pytest.raises(ValueError, match="matrix"):
            call(torch.zeros(2, 3, 4))
        with pytest.raises(ValueError, match="at least two rows"):
            call(X[:1])
        with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
            call(bad)
        with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
            call(inf)
        for k in (0, 4, -2, 1.0, 2.5):
            with pytest.raises(ValueError, match="n_components"):
                call(X, n_components=k)
        with pytest.raises(NotImplementedError, match="mle"):
            call(X, n_components="mle")
        with pytest.raises(NotImplementedError, match="4096"):
            call(np.zeros((3, 4097), dtype=np.float32))
    with pytest.raises(ValueError, match="at least two rows"):
        reduce.StandardScaler().fit(X[:1])
    with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
        reduce.StandardScaler().fit_transform(bad)
    with pytest.raises(ValueError, match="Input X contains NaN or infinity."):
        reduce.compute_pca({"features": bad, "id": np.arange(6)})
    with pytest.raises(RuntimeError, match="not fitted"):
        reduce.PCA().transform(X)


def test_no_cpu_fallback(monkeypatch):
    from viscy_amd import ops, reduce

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # what a machine without a HIP device answers
    X = np.random.RandomState(1).randn(5, 3).astype(np.float32)
    for call in (lambda: reduce.compute_pca(X), lambda: reduce.PCA(2).fit(X), lambda: reduce.StandardScaler().fit(X),
                 lambda: reduce.compute_pca(torch.from_numpy(X), n_components=2, normalize_features=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.col_moments(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.gram_centered(torch.zeros(4, 3), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.center_project(torch.zeros(4, 3), torch.zeros(3, dtype=torch.float64), torch.zeros(2, 3))


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_size_queries_equal_their_formulas():
    from viscy_amd import _lib

    l = _lib.lib()
    shapes = [(2, 1), (2, 4), (33, 33), (129, 128), (257, 260), (511, 132), (512, 132), (513, 132), (1300, 768), (100000, 768),
              (1000000, 768), (10 ** 6, 4096), (2 ** 31 - 1, 64), (5000, 129), (123457, 1000)]
    for n, d in shapes:
        tiles, pairs, splits, rps = RP.gram_plan(n, d)
        assert l.vsx_gram_rows_per_split(n, d) == rps and rps % RP.R == 0 and (splits - 1) * rps < n <= splits * rps, (n, d)
        assert l.vsx_gram_ws_bytes(n, d) == RP.gram_ws_bytes(n, d) == splits * pairs * 128 * 128 * 8, (n, d)
        assert l.vsx_col_moments_ws_bytes(n, d) == RP.moments_ws_bytes(n, d), (n, d)
    # the launch fills the chip at the product's width, and the workspace stays O(splits d^2)
    assert RP.gram_plan(10 ** 6, 768)[1:3] == (21, 24) and l.vsx_gram_ws_bytes(10 ** 6, 768) == 24 * 21 * 131072   # 504 <= 512 workgroups
    assert l.vsx_gram_ws_bytes(10 ** 6, 4096) == 528 * 131072   # 528 tile pairs: one split
    for n, d in ((1, 4), (0, 4), (2 ** 31, 4), (8, 0), (8, 4097), (-3, 4)):
        assert l.vsx_gram_ws_bytes(n, d) == 0 and l.vsx_gram_rows_per_split(n, d) == 0 and l.vsx_col_moments_ws_bytes(n, d) == 0, (n, d)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """VSX_CHECK errors: nothing is launched, so this runs without a device (the pointers are host arrays no kernel ever sees)"""
    from viscy_amd import _lib

    l = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 40
    need_m, need_g = l.vsx_col_moments_ws_bytes(8, 4), l.vsx_gram_ws_bytes(8, 4)
    assert need_m == 32 and need_g == 131072
    for fn, need, name in ((l.vsx_col_moments, need_m, b"vsx_col_moments"), (l.vsx_gram_centered, need_g, b"vsx_gram_centered")):
        for args, msg in (((p, 1, 4, p, p, p, big, None), b"n=1 must be in [2, 2^31)"),
                          ((p, 1 << 31, 4, p, p, p, big, None), b"n=2147483648 must be in [2, 2^31)"),
                          ((p, 8, 0, p, p, p, big, None), b"d=0 must be in [1, 4096]"),
                          ((p, 8, 4097, p, p, p, big, None), b"d=4097 must be in [1, 4096]"),
                          ((None, 8, 4, p, p, p, big, None), b"null argument"),
                          ((p, 8, 4, None, p, p, big, None), b"null argument"),
                          ((p, 8, 4, p, None, p, big, None), b"null argument"),
                          ((p, 8, 4, p, p, None, big, None), b"null argument"),
                          ((p + 2, 8, 4, p, p, p, big, None), b"4-byte aligned"),
                          ((p, 8, 4, p + 4, p, p, big, None), b"8-byte aligned"),
                          ((p, 8, 4, p, p, p + 4, big, None), b"8-byte aligned"),
                          ((p, 8, 4, p, p, p, need - 1, None), b"bytes (got %d)" % (need - 1))):
            assert fn(*args) == 1 and msg in l.vsx_last_error() and name in l.vsx_last_error(), (name, args[1:3], l.vsx_last_error())
    for args, msg in (((p, 1, 4, p, p, 2, p, None), b"n=1 must be in [2, 2^31)"),
                      ((p, 8, 5000, p, p, 2, p, None), b"d=5000 must be in [1, 4096]"),
                      ((p, 8, 4, p, p, 0, p, None), b"k=0 must be in [1,"),
                      ((p, 8, 4, p, p, -1, p, None), b"k=-1 must be in [1,"),
                      ((p, 8, 4, None, p, 2, p, None), b"null argument"),
                      ((p, 8, 4, p, None, 2, p, None), b"null argument"),
                      ((p, 8, 4, p, p, 2, None, None), b"null argument"),
                      ((p, 8, 4, p + 4, p, 2, p, None), b"8-byte aligned"),
                      ((p, 8, 4, p, p + 1, 2, p, None), b"4-byte aligned")):
        assert l.vsx_center_project(*args) == 1 and msg in l.vsx_last_error(), (args[1:3], l.vsx_last_error())


def test_integer_fixtures_are_exact_in_float64():
    """what the GPU tests compare against bit for bit: integer means, and block sums of centred products below 2^24"""
    for N, d in ((2, 4), (33, 33), (513, 132)):
        x, mean, m2, gram = RP.int_fixture(N, d)
        x64 = x.astype(np.float64)
        assert np.abs(x).max() <= 1024 and (x64.sum(0) / N == mean).all()
        c = x64 - mean
        assert (np.abs(c) <= RP.VMAX).all() and ((c * c).sum(0) == m2).all() and (c.T @ c == gram).all()
        for r0 in range(0, N, RP.R):
            assert (np.abs(c[r0:r0 + RP.R]).T @ np.abs(c[r0:r0 + RP.R])).max() < 2 ** 24
        assert (RP.gram_f32_blocks(x, mean.astype(np.float64)) == gram).all()   # the emulation is exact on them too
    w = RP.int_weights(129, 768)
    assert np.abs(w).max() <= 3 and 768 * RP.VMAX * 3 < 2 ** 24
