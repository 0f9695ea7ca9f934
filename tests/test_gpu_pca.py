"""GPU: viscy_amd.reduce and the kernels of csrc/pca.hip under it.

Exact (integer fixtures of tests/ref_pca.py: integer column means, centred products whose fp32 block sums stay below 2^24, so
float64 is exact).  vsx_col_moments and vsx_gram_centered equal the integer mean, m2 and Gram bit for bit at every (N, d) of the
case table (the minimum, d % 4 != 0, one tile, a second tile of 4 columns, three tiles with off-diagonal pairs, 21 tile pairs,
both sides of a split and of a block, a ragged multi-block second split), the Gram is exactly symmetric, two runs are bit-identical
and a run on poisoned allocations equals a clean one; a view 4 bytes off the 16-byte grid (scalar loads) gives the same bits.
vsx_center_project equals float64 on integer x, integer mean and small-integer w at k = 1, 127, 128, 129 for d = 33 and 768.

Accuracy (tests/golden/pca.pt), against the float64 restatement: explained_variance_ (relative to the largest), the ratio and
1 - |cos| of the compared components within 4 x max(err_ref, gram_err_f32), pc_features within 4 x max(err_ref, the emulation's
projection error), each quantity against its own pair of numbers; signs equal to the reference's wherever svd_flip's choice is
decided; n_components_ equal to the reference's.  The factor 4 is the margin test_gpu_mmd.py gives a device result over the
reference's own float32 error: the summation orders differ, the arithmetic class does not.

Interface: numpy array, host tensor and device tensor give the same bytes; the mapping input yields the reference's column order;
StandardScaler against sklearn's recorded statistics; PCA.transform on a slice equals fit_transform's rows bit for bit and held-out
rows agree with float64."""

import functools

import numpy as np
import pytest
import torch

from tests import ref_pca as RP
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = {True: "norm", False: "raw"}
CASE_MODES = [(name, nm) for name in RP.CASES for nm in RP.NORMALIZE]


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("pca.pt")["cases"]


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("N,d", RP.exact_shapes())
def test_moments_and_gram_are_bit_equal_to_float64(N, d):
    from viscy_amd import debug, ops

    x, mean, m2, gram = RP.int_fixture(N, d)
    xd = torch.from_numpy(x.copy()).to(DEV)
    mu, s2 = ops.col_moments(xd)
    assert mu.dtype == torch.float64 and s2.dtype == torch.float64
    assert np.array_equal(mu.cpu().numpy(), mean.astype(np.float64))
    assert np.array_equal(s2.cpu().numpy(), m2.astype(np.float64))
    G = ops.gram_centered(xd, mu)
    assert G.dtype == torch.float64 and G.shape == (d, d)
    assert np.array_equal(G.cpu().numpy(), gram.astype(np.float64))
    assert torch.equal(G, G.t())
    assert torch.equal(ops.gram_centered(xd, mu), G)                           # two runs
    again = ops.col_moments(xd)
    assert torch.equal(again[0], mu) and torch.equal(again[1], s2)
    with debug.poison_empty():                                                 # the calls initialise what they read
        pm, ps = ops.col_moments(xd)
        assert torch.equal(pm, mu) and torch.equal(ps, s2)
        assert torch.equal(ops.gram_centered(xd, mu), G)
    # 4 bytes off the 16-byte grid: d % 4 == 0 takes the scalar loads too
    flat = torch.empty(N * d + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(N, d)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4
    vm, vs = ops.col_moments(view)
    assert torch.equal(vm, mu) and torch.equal(vs, s2) and torch.equal(ops.gram_centered(view, mu), G)


def test_split_plan_of_the_exact_shapes():
    from viscy_amd import ops

    r = RP.R132
    assert [ops.gram_rows_per_split(n, 132) for n in (r - 1, r, r + 1, r + RP.R + 2)] == [r] * 4
    assert ops.gram_rows_per_split(1300, 768) == RP.gram_plan(1300, 768)[3] == 512 and RP.gram_plan(1300, 768)[2] == 3


@pytest.mark.parametrize("d", RP.PROJECT_D)
@pytest.mark.parametrize("k", RP.PROJECT_K)
def test_center_project_is_bit_equal_to_float64(k, d):
    from viscy_amd import debug, ops

    x, mean, _, _ = RP.int_fixture(RP.PROJECT_N, d, seed=1)
    w = RP.int_weights(k, d)
    want = (x.astype(np.float64) - mean) @ w.astype(np.float64).T
    assert np.abs(want).max() < 2 ** 24
    xd, md, wd = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(mean.astype(np.float64)).to(DEV), torch.from_numpy(w).to(DEV)
    z = ops.center_project(xd, md, wd)
    assert z.dtype == torch.float32 and z.shape == (RP.PROJECT_N, k)
    assert np.array_equal(z.cpu().numpy().astype(np.float64), want)
    with debug.poison_empty():
        assert torch.equal(ops.center_project(xd, md, wd), z)
    flat = torch.empty(RP.PROJECT_N * d + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(RP.PROJECT_N, d)
    view.copy_(xd)
    assert torch.equal(ops.center_project(view, md, wd), z)


# ------------------------------------------------------------------------------------------------ accuracy
@functools.lru_cache(maxsize=None)
def device_fit(name, normalize):
    """PCA(...).fit_transform on the case, once"""
    from viscy_amd.reduce import PCA

    est = PCA(n_components=RP.CASES[name]["k"], normalize_features=normalize, random_state=42)
    Z = est.fit_transform(RP.build(name))
    Z.setflags(write=False)
    return est, Z


@pytest.mark.parametrize("name,normalize", CASE_MODES)
def test_fit_against_the_restatement_and_the_reference(name, normalize):
    c, e = RP.CASES[name], golden()[name][KEY[normalize]]
    ours = RP.restatement(name, normalize)
    idx = RP.compared(name, normalize)
    est, Z = device_fit(name, normalize)
    k = ours["n_components"]
    assert est.n_components_ == k == e["n_components"]
    assert Z.dtype == np.float32 and Z.shape == (c["N"], k)
    for a in (est.components_, est.explained_variance_, est.explained_variance_ratio_, est.singular_values_, est.mean_):
        assert a.dtype == np.float64
    assert est.components_.shape == (k, c["d"])
    err = RP.errors(dict(explained_variance=est.explained_variance_, ratio=est.explained_variance_ratio_, components=est.components_, Z=Z),
                    ours, idx)
    bound = tuple(4 * max(a, b) for a, b in zip(e["err_ref"], e["gram_err_f32"]))
    print(f"\n{name} {KEY[normalize]}: variance {err[0]:.3e} (bound {bound[0]:.3e})  1 - |cos| {err[1]:.3e} (bound {bound[1]:.3e})  "
          f"projection {err[2]:.3e} (bound {bound[2]:.3e})")
    assert err[0] <= bound[0] and err[1] <= bound[1] and err[2] <= bound[2]
    dec = RP.decided(name, normalize)   # every compared component but those of two standardised rows (tests/test_pca_cpu.py)
    assert RP.signs_agree(est.components_, ours, dec)
    assert RP.signs_agree(e["components"].numpy(), dict(components=est.components_), dec)   # the reference's
    np.testing.assert_allclose(est.singular_values_, np.sqrt(est.explained_variance_ * (c["N"] - 1)), rtol=1e-14)
    assert abs(est.noise_variance_ - ours["noise_variance"]) <= bound[0] * ours["all_variance"][0]


# ------------------------------------------------------------------------------------------------ interface
def test_compute_pca_takes_arrays_tensors_and_mappings():
    import pandas as pd

    from viscy_amd.reduce import compute_pca

    name = "n300_d132_k8"
    x = RP.build(name)
    est, Z = device_fit(name, True)
    pc, df = compute_pca(x, n_components=8)
    assert isinstance(pc, np.ndarray) and pc.dtype == np.float32 and np.array_equal(pc, Z)      # normalize_features defaults to True
    assert isinstance(df, pd.DataFrame) and list(df.columns) == [f"PC{i + 1}" for i in range(8)] and np.array_equal(df["PC3"].to_numpy(), pc[:, 2])
    for other in (torch.from_numpy(x.copy()), torch.from_numpy(x.copy()).to(DEV), x.astype(np.float64)):
        assert np.array_equal(compute_pca(other, n_components=8)[0], pc)
    raw = compute_pca(x, 8, False)[0]
    assert np.array_equal(raw, device_fit(name, False)[1]) and not np.array_equal(raw, pc)
    n = len(x)
    meta = {"track_id": np.arange(n) % 7, "features": x, "t": np.arange(n), "fov_name": np.array([f"A/1/{i % 3}" for i in range(n)]),
            "id": np.arange(n) + 100, "projections": x[:, :4]}
    pc2, df2 = compute_pca(meta, n_components=8)
    assert np.array_equal(pc2, pc)
    assert list(df2.columns) == ["id", "fov_name", "t", "track_id"] + [f"PC{i + 1}" for i in range(8)]
    assert df2["id"].iloc[5] == 105 and df2["fov_name"].iloc[4] == "A/1/1"
    pc3, df3 = compute_pca({"features": torch.from_numpy(x.copy()).to(DEV), "t": torch.arange(n)}, n_components=8)
    assert np.array_equal(pc3, pc) and list(df3.columns)[:2] == ["t", "PC1"]
    assert compute_pca(x)[0].shape == (300, 132)                                                  # None: min(N, D)


@pytest.mark.parametrize("name", ["n33_d33_all", "n300_d132_const", "n1300_d768_k8"])
def test_standard_scaler_against_the_recorded_statistics(name):
    from viscy_amd.reduce import StandardScaler

    g, x = golden()[name], RP.build(name)
    sc = StandardScaler()
    out = sc.fit_transform(x)
    assert sc.n_samples_seen_ == len(x) and out.dtype == np.float32 and out.shape == x.shape
    np.testing.assert_allclose(sc.mean_, g["scaler_mean"].numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sc.var_, g["scaler_var"].numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sc.scale_, g["scaler_scale"].numpy(), rtol=1e-9)
    # sklearn subtracts a float32 mean from float32 data: 2^-24 (|mean| + |x|) / scale apart at most, plus the two roundings here
    head, x4 = g["scaled_head"].numpy().astype(np.float64), x[:4].astype(np.float64)
    tol = 2.0 ** -23 * (np.abs(sc.mean_) + np.abs(x4)) / sc.scale_ + 4 * 2.0 ** -24 * np.abs(head) + 1e-30
    assert (np.abs(out[:4] - head) <= tol).all()
    want = (x.astype(np.float64) - sc.mean_) / sc.scale_
    assert np.abs(out - want).max() <= 3 * 2.0 ** -24 * np.abs(want).max()
    assert np.array_equal(sc.transform(torch.from_numpy(x[7:8].copy())), out[7:8])                # a single row


def test_transform_is_fit_transforms_arithmetic():
    from viscy_amd.reduce import PCA

    name = "n1300_d768_k8"
    x = RP.build(name)
    for nm in RP.NORMALIZE:
        est, Z = device_fit(name, nm)
        assert np.array_equal(est.transform(x[100:400]), Z[100:400])           # another row tile, the same dots
        assert np.array_equal(est.transform(torch.from_numpy(x[1299:].copy()).to(DEV)), Z[1299:])
        held = PCA(n_components=8, normalize_features=nm).fit(x[:1000])
        got = held.transform(x[1000:])
        f = held.fit_
        want = ((x[1000:].astype(np.float64) - f.data_mean) / f.scale) @ f.components_.T
        e = golden()[name][KEY[nm]]
        assert np.abs(got - want).max() <= 4 * max(e["err_ref"][2], e["gram_err_f32"][2]) * np.abs(want).max()


def test_ops_refuse_what_they_do_not_serve():
    from viscy_amd import ops

    x = torch.zeros((8, 4), device=DEV)
    m = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError, match="float64"):
        ops.gram_centered(x, m.float())
    with pytest.raises(TypeError, match="float32"):
        ops.col_moments(x.double())
    with pytest.raises(TypeError, match=r"\(k, 4\)"):
        ops.center_project(x, m, torch.zeros((2, 5), device=DEV))
    with pytest.raises(RuntimeError, match=r"n=1 must be in \[2, 2\^31\)"):
        ops.col_moments(x[:1])
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.gram_centered(x.cpu(), m)
