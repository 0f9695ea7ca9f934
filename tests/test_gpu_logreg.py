"""GPU: viscy_amd.linear_classifier and the kernels under it (csrc/logreg.hip, vsx_gram_scaled of csrc/pca.hip).

Exact (integer fixtures, float64 is exact): vsx_gram_scaled on integer x in [-15, 15] and q in {0, 1, 2} (a block's fp32 sum stays
below 128 * 30^2 < 2^24) equals float64 bit for bit and is exactly symmetric at every (N, d) of tests/ref_pca.py's table plus d = 1,
and with q = 1 and a mean it is vsx_gram_centered bit for bit; vsx_wcolsum with integer weights at m = 1, 2, 4; vsx_logreg_rows'
margins for integer w and b, and at w = 0 sigma = 1/2: r = -c y / 2, s = c / 4 and q exact, loss = c log 2 within 2 ulp.  For all
three: two runs are bit-identical, a run on poisoned allocations equals a clean one, and a view 4 bytes off the 16-byte grid (the
scalar loads) gives the same bits.

Accuracy of the row pass on real w with |m| up to 40: z within 2 gamma_d sum_j |x_ij w_j| of numpy (gamma_d = d 2^-53, one for each
of the two float64 summation orders); loss, r, s against numpy at the device's own z within 16 ulp (2^-49 relative: the formulas
have no cancellation, exp is documented at 1 ulp and log1p at 2); q within 1 fp32 ulp of sqrt(s).  The measured worst cases are
printed (pytest -s) and recorded in profiles/linear_classifier_perf.txt.

Estimator, per case of tests/ref_logreg.py: the float64 numpy gradient at (coef_, intercept_) is within 2 eps |g(0)| (2: the device
gradient's own rounding), hence for liblinear's objective (Hessian >= I) |u - u*| is; against sklearn as run (default tol),
|u - u_sk| <= |u_sk - u*| + that; predict equals sklearn's on every decided row (at most 2 % are not); predict_proba within 1/4 of
the row bound; rows sum to 1; numpy, host-tensor and device-tensor inputs give the same bytes.

Pipeline: train_linear_classifier / predict_with_classifier on a duck-typed adata of 600 x 96 with string labels (a class of 40),
with and without scaling, PCA(8) and groups: key sets and val_outputs as the reference's; the count metrics equal the recorded
ones (every row of the fixture is decided by 10 x the bound); AUROC within 4 x the recorded |default - tol=1e-10| difference with a
floor of one swapped pair."""

import collections
import functools

import numpy as np
import pytest
import torch

from tests import ref_logreg as RL
from tests import ref_pca as RP
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("logreg.pt")


def off_grid(xd):
    """a copy of xd 4 bytes off the 16-byte grid"""
    flat = torch.empty(xd.numel() + 1, dtype=xd.dtype, device=DEV)
    view = flat[1:].view(xd.shape)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4
    return view


def int_rows(N, d, seed):
    rng = np.random.RandomState(3000 + seed)
    return np.ascontiguousarray(rng.randint(-15, 16, (N, d)).astype(np.float32)), rng


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("N,d", RP.exact_shapes() + [(300, 1)])
def test_gram_scaled_is_bit_equal_to_float64(N, d):
    from viscy_amd import debug, ops

    x, rng = int_rows(N, d, N + d)
    q = rng.randint(0, 3, N).astype(np.float32)
    qx = x.astype(np.float64) * q[:, None].astype(np.float64)
    want = qx.T @ qx
    xd, qd = torch.from_numpy(x).to(DEV), torch.from_numpy(q).to(DEV)
    G = ops.gram_scaled(xd, qd)
    assert G.dtype == torch.float64 and G.shape == (d, d)
    assert np.array_equal(G.cpu().numpy(), want)
    assert torch.equal(G, G.t())
    assert torch.equal(ops.gram_scaled(xd, qd), G)
    with debug.poison_empty():
        assert torch.equal(ops.gram_scaled(xd, qd), G)
    assert torch.equal(ops.gram_scaled(off_grid(xd), off_grid(qd)), G)
    # q = 1 and a mean: the centred Gram, bit for bit
    xi, mean, _, gram = RP.int_fixture(N, d)
    xi_d, mu = torch.from_numpy(xi.copy()).to(DEV), torch.from_numpy(mean.astype(np.float64)).to(DEV)
    ones = torch.ones(N, dtype=torch.float32, device=DEV)
    Gc = ops.gram_centered(xi_d, mu)
    assert torch.equal(ops.gram_scaled(xi_d, ones, mu), Gc) and np.array_equal(Gc.cpu().numpy(), gram.astype(np.float64))


@pytest.mark.parametrize("m", [1, 2, 4])
@pytest.mark.parametrize("N,d", [(2, 1), (40, 5), (1300, 768), (5000, 132)])
def test_wcolsum_is_bit_equal_to_float64(N, d, m):
    from viscy_amd import debug, ops

    x, rng = int_rows(N, d, 7 * N + d + m)
    v = rng.randint(-8, 9, (m, N)).astype(np.float64)
    want = v @ x.astype(np.float64)
    xd, vd = torch.from_numpy(x).to(DEV), torch.from_numpy(v).to(DEV)
    out = ops.wcolsum(xd, vd)
    assert out.dtype == torch.float64 and out.shape == (m, d)
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(ops.wcolsum(xd, vd), out)
    with debug.poison_empty():
        assert torch.equal(ops.wcolsum(xd, vd), out)
    assert torch.equal(ops.wcolsum(off_grid(xd), vd), out)


@pytest.mark.parametrize("N,d", [(2, 1), (40, 5), (300, 132), (1300, 768), (5000, 260)])
def test_logreg_rows_exact_parts(N, d):
    from viscy_amd import debug, ops

    x, rng = int_rows(N, d, 13 * N + d)
    w = rng.randint(-4, 5, d).astype(np.float64)
    b = 3.0
    labels = rng.randint(0, 3, N).astype(np.int32)
    cp, cn = 1.7, 0.3
    xd, wd, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(labels).to(DEV)
    want_z = x.astype(np.float64) @ w + b
    z = ops.logreg_margins(xd, wd, b)
    assert z.dtype == torch.float64 and np.array_equal(z.cpu().numpy(), want_z)
    full = ops.logreg_rows(xd, wd, b, ld, 2, cp, cn, margins=True)
    assert torch.equal(full["z"], z)                                           # the fit's dots are the decision function's
    for run in ("again", "poisoned", "off_grid"):
        if run == "poisoned":
            with debug.poison_empty():
                other, oz = ops.logreg_rows(xd, wd, b, ld, 2, cp, cn, margins=True), ops.logreg_margins(xd, wd, b)
        else:
            xx = off_grid(xd) if run == "off_grid" else xd
            other, oz = ops.logreg_rows(xx, wd, b, ld, 2, cp, cn, margins=True), ops.logreg_margins(xx, wd, b)
        assert torch.equal(oz, z)
        for key in ("z", "r", "s", "q", "sums"):
            assert torch.equal(other[key], full[key]), (run, key)
    assert torch.equal(ops.logreg_rows(xd, wd, b, ld, 2, cp, cn, derivatives=False)["sums"], full["sums"])   # a line-search trial
    # w = 0: sigma = 1/2
    zero = ops.logreg_rows(xd, torch.zeros_like(wd), 0.0, ld, 2, cp, cn, margins=True)
    pos = labels == 2
    c = np.where(pos, cp, cn)
    assert np.array_equal(zero["z"].cpu().numpy(), np.zeros(N))
    assert np.array_equal(zero["r"].cpu().numpy(), -c * np.where(pos, 1.0, -1.0) * 0.5)
    assert np.array_equal(zero["s"].cpu().numpy(), c * 0.5 * 0.5)
    assert np.array_equal(zero["q"].cpu().numpy(), np.sqrt(c * 0.25).astype(np.float32))
    sums = zero["sums"].cpu().numpy()
    want = np.array([np.sum(c) * np.log(2.0), np.sum(-c * np.where(pos, 1.0, -1.0) * 0.5), np.sum(c) * 0.25])
    assert (np.abs(sums - want) <= N * ULP * np.array([np.sum(c), np.sum(c), np.sum(c)])).all()
    one = ops.logreg_rows(xd[:2].contiguous(), torch.zeros_like(wd), 0.0, ld[:2].contiguous(), int(labels[0]), cp, cn)
    lone = one["sums"].cpu().numpy()[0]                                        # two rows: c_0 log 2 + c_1 log 2, each within 2 ulp
    c2 = np.where(labels[:2] == labels[0], cp, cn)
    assert abs(lone - c2.sum() * np.log(2.0)) <= 3 * ULP * c2.sum() * np.log(2.0)


def test_ops_refuse_what_they_do_not_serve():
    from viscy_amd import ops

    x = torch.zeros((8, 4), device=DEV)
    w = torch.zeros(4, dtype=torch.float64, device=DEV)
    lab = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="float64"):
        ops.logreg_margins(x, w.float(), 0.0)
    with pytest.raises(TypeError, match="int32"):
        ops.logreg_rows(x, w, 0.0, lab.long(), 1, 1.0, 1.0)
    with pytest.raises(TypeError, match="1 <= m <= 4"):
        ops.wcolsum(x, torch.zeros((5, 8), dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        ops.gram_scaled(x, torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match=r"n=1 must be in \[2, 2\^31\)"):
        ops.logreg_margins(x[:1], w, 0.0)


# ------------------------------------------------------------------------------------------------ accuracy of the row pass
def test_rows_accuracy_on_real_weights():
    from viscy_amd import ops

    x, y = RL.build("bin_n1300_d768_bal")
    x64 = x.astype(np.float64)
    rng = np.random.RandomState(77)
    w = rng.randn(x.shape[1])
    w *= 40.0 / np.abs(x64 @ w).max()                                          # |m| up to 40
    b, cp, cn = 0.25, 1.3, 0.6
    xd = torch.from_numpy(x.copy()).to(DEV)
    out = ops.logreg_rows(xd, torch.from_numpy(w).to(DEV), b, torch.from_numpy(y.astype(np.int32)).to(DEV), 1, cp, cn,
                          margins=True)
    z, r, s, q = (out[k].cpu().numpy() for k in ("z", "r", "s", "q"))
    d = x.shape[1]
    bound_z = 2.0 * d * 2.0 ** -53 * (np.abs(x64) @ np.abs(w) + abs(b))
    err_z = np.abs(z - (x64 @ w + b))
    assert np.abs(z).max() > 39.0
    yy, c = np.where(y == 1, 1.0, -1.0), np.where(y == 1, cp, cn)
    m = yy * z
    e = np.exp(-np.abs(m))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sig, om = np.where(m >= 0, big, small), np.where(m >= 0, small, big)
    loss_i = c * (np.log1p(e) + np.maximum(-m, 0.0))
    want_r, want_s = -c * yy * om, c * sig * om
    ulp_r = np.abs(r - want_r) / (ULP * np.abs(want_r))
    ulp_s = np.abs(s - want_s) / (ULP * np.abs(want_s))
    sums = out["sums"].cpu().numpy()
    # the sums carry the per-row error and a float64 summation of n terms
    n = len(y)
    ulp_sums = np.abs(sums - np.array([loss_i.sum(), want_r.sum(), want_s.sum()])) / (ULP * np.array([loss_i.sum(), np.abs(want_r).sum(), want_s.sum()]))
    sq = np.sqrt(s)
    ulp_q = np.abs(q.astype(np.float64) - sq) / np.spacing(sq.astype(np.float32)).astype(np.float64)
    print(f"\nrows accuracy (n={n}, d={d}, |m| <= {np.abs(m).max():.1f}): z err / bound {np.max(err_z / bound_z):.3f}; r {ulp_r.max():.2f} ulp, "
          f"s {ulp_s.max():.2f} ulp (bound 16); sums loss / r / s {ulp_sums[0]:.1f} / {ulp_sums[1]:.1f} / {ulp_sums[2]:.1f} ulp of sum |.| "
          f"(bound 16 + n); q {ulp_q.max():.3f} fp32 ulp (bound 1)")
    assert (err_z <= bound_z).all()
    assert ulp_r.max() <= 16.0 and ulp_s.max() <= 16.0
    assert (ulp_sums <= 16.0 + n).all()
    assert ulp_q.max() <= 1.0
    # the loss per row, through a two-row call: the second row's loss is the sums' difference from the first's; read it directly
    # instead from single-problem sums at n = 2
    worst = 0.0
    for i in (int(np.argmax(m)), int(np.argmin(m)), int(np.argmin(np.abs(m))), 0):
        j = i + 1 if i + 1 < n else i - 1
        pair = ops.logreg_rows(xd[[i, j]].contiguous(), torch.from_numpy(w).to(DEV), b,
                               torch.from_numpy(y[[i, j]].astype(np.int32)).to(DEV), 1, cp, cn, margins=True)
        assert torch.equal(pair["z"].cpu(), torch.from_numpy(z[[i, j]]))       # a row's dot does not depend on its neighbours
        want = loss_i[i] + loss_i[j]
        worst = max(worst, abs(float(pair["sums"][0]) - want) / (ULP * want))
    print(f"loss of a pair of rows: {worst:.2f} ulp (bound 17: 16 per row and the one add)")
    assert worst <= 17.0


# ------------------------------------------------------------------------------------------------ estimator
@functools.lru_cache(maxsize=None)
def device_fit(name):
    from viscy_amd.linear_classifier import LogisticRegression

    x, y = RL.build(name)
    est = LogisticRegression(**RL.CASES[name]["params"]).fit(x, y)
    return est


@pytest.mark.parametrize("name", list(RL.CASES))
def test_estimator_against_the_optimum_and_sklearn(name):
    x, y = RL.build(name)
    x64, params, g = x.astype(np.float64), RL.CASES[name]["params"], golden()["cases"][name]
    est = device_fit(name)
    K = len(np.unique(y))
    d = x.shape[1]
    assert np.array_equal(est.classes_, np.unique(y)) and est.n_features_in_ == d
    assert est.coef_.shape == ((1 if K == 2 else K), d) and est.coef_.dtype == np.float64 and est.intercept_.shape == (len(est.coef_),)
    if not params.get("fit_intercept", True):
        assert np.array_equal(est.intercept_, np.zeros(len(est.coef_)))
    U = RL.stack_u(est.coef_, est.intercept_, params, d)
    U_sk = RL.stack_u(g["default"]["coef"].numpy(), g["default"]["intercept"].numpy(), params, d)
    liblinear = params["solver"] == "liblinear"
    for k, prob in enumerate(RL.problems(params, y)):
        u_star, g0, lam, eps = RL.optimum(name)[k]
        gn = float(np.linalg.norm(RL.gradient(x64, prob, params, est.coef_[k], est.intercept_[k])))
        dist, dist_sk = float(np.linalg.norm(U[k] - u_star)), float(np.linalg.norm(U[k] - U_sk[k]))
        print(f"\n{name}[{k}]: {est.n_iter_[k]} iterations, {est.fit_info_[k].n_evals} trials; |g| / |g(0)| {gn / g0:.2e} (bound {2 * eps:.1e}); "
              f"|u - u*| {dist:.2e} (bound {2 * eps * g0:.2e}); |u - u_sk| {dist_sk:.2e} (|u_sk - u*| {g['dist_default'][k]:.2e})")
        assert est.fit_info_[k].converged
        assert gn <= 2.0 * eps * g0
        own = 2.0 * eps * g0 if liblinear else 2.0 * (2.0 * eps * g0) / min(lam, 1.0)   # Hessian >= I | >= lambda_min near u*
        assert dist <= own + 1e-14 * np.linalg.norm(u_star)
        assert dist_sk <= g["dist_default"][k] + own + 1e-14 * np.linalg.norm(u_star)
    # labels and probabilities against sklearn as run
    bound = RL.row_bound(x, max(g["dist_default"]))
    z_sk = g["default"]["decision"].numpy()
    dec = RL.decided(z_sk, bound)
    assert np.mean(~dec) <= RL.UNDECIDED_CAP and np.mean(~dec) == pytest.approx(g["undecided"])
    pred = est.predict(x)
    assert np.array_equal(pred[dec], g["default"]["pred"].numpy()[dec])
    proba = est.predict_proba(x)
    assert proba.dtype == np.float64 and proba.shape == (len(y), K)
    err_p = np.abs(proba - g["default"]["proba"].numpy()).max(axis=1)
    print(f"{name}: undecided {np.mean(~dec):.4f}; max |proba - sklearn's| / (bound / 4) = {np.max(err_p / (0.25 * bound)):.3e}")
    assert (err_p <= 0.25 * bound).all()
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= 4 * ULP
    zf = est.decision_function(x)
    assert zf.dtype == np.float64 and zf.shape == z_sk.shape
    assert np.array_equal(est.predict_log_proba(x), np.log(proba))
    assert est.score(x, y) == np.mean(pred == y)


@pytest.mark.parametrize("name", ["bin_n40_d5", "ovr3_n600_d96_bal"])
def test_inputs_numpy_host_tensor_device_tensor_give_the_same_bytes(name):
    from viscy_amd.linear_classifier import LogisticRegression

    x, y = RL.build(name)
    est = device_fit(name)
    want_p, want_z = est.predict_proba(x), est.decision_function(x)
    for other in (torch.from_numpy(x.copy()), torch.from_numpy(x.copy()).to(DEV), x.astype(np.float64)):
        e2 = LogisticRegression(**RL.CASES[name]["params"]).fit(other, y)
        assert np.array_equal(e2.coef_, est.coef_) and np.array_equal(e2.intercept_, est.intercept_) and np.array_equal(e2.n_iter_, est.n_iter_)
        assert np.array_equal(e2.predict_proba(other), want_p) and np.array_equal(e2.decision_function(other), want_z)
    assert np.array_equal(est.decision_function(x[5:6]), want_z[5:6])          # a single row
    words = np.asarray(["no", "yes", "zz"], dtype=object)
    e3 = LogisticRegression(**RL.CASES[name]["params"]).fit(x, words[y])       # string labels: the same problems
    assert np.array_equal(e3.coef_, est.coef_) and np.array_equal(e3.predict(x), words[est.predict(x)])


# ------------------------------------------------------------------------------------------------ pipeline
COUNT_KEYS = ("accuracy", "precision", "recall", "f1", "support")


@functools.lru_cache(maxsize=None)
def device_pipeline(cfg):
    from viscy_amd.linear_classifier import train_linear_classifier

    scal, use_pca, k, grouped, frac = RL.PIPE_CONFIGS[cfg]
    groups = RL.pipe_arrays()[2]
    return train_linear_classifier(RL.pipe_adata(), RL.pipe_task(), use_scaling=scal, use_pca=use_pca, n_pca_components=k,
                                   classifier_params=dict(RL.PIPE_PARAMS), split_train_data=frac, random_seed=42, groups=groups if grouped else None)


@pytest.mark.parametrize("cfg", list(RL.PIPE_CONFIGS))
def test_train_linear_classifier_against_the_reference(cfg):
    g = golden()["pipeline"][cfg]
    pipe, metrics, val = device_pipeline(cfg)
    scal, use_pca, k, grouped, frac = RL.PIPE_CONFIGS[cfg]
    assert set(metrics) == set(g["metrics"])
    assert list(val) == ["y_val", "y_val_proba", "classes"] and val["classes"] == g["classes"] == list(RL.PIPE_CLASSES)
    assert (pipe.scaler is not None) == scal and (pipe.pca is not None) == use_pca and pipe.task == RL.pipe_task()
    assert pipe.config == {"task": RL.pipe_task(), "use_scaling": scal, "use_pca": use_pca, "n_pca_components": k,
                           "classifier_params": dict(RL.PIPE_PARAMS), "split_train_data": frac, "random_seed": 42}
    if frac >= 1.0:
        assert val["y_val"] is None and val["y_val_proba"] is None and not [key for key in metrics if key.startswith("val_")]
    else:
        assert list(val["y_val"]) == g["y_val"]                                # the split's rows, in its order
        assert val["y_val_proba"].shape == tuple(g["y_val_proba"].shape) and np.abs(val["y_val_proba"].sum(axis=1) - 1.0).max() <= 4 * ULP
    all_counts = collections.Counter(RL.pipe_arrays()[1])
    val_counts = collections.Counter(val["y_val"] if frac < 1.0 else [])     # the train part is the rest
    for key, want in g["metrics"].items():
        if key.endswith(COUNT_KEYS):
            assert metrics[key] == pytest.approx(want, rel=1e-12, abs=1e-12), key
            if key.endswith("support"):
                assert isinstance(metrics[key], int)
        else:
            assert key.endswith("auroc")
            counts = val_counts if key.startswith("val_") else {c: all_counts[c] - val_counts[c] for c in RL.PIPE_CLASSES}
            n_part = sum(counts.values())
            cls = [c for c in RL.PIPE_CLASSES if key == f"val_{c}_auroc"] or list(RL.PIPE_CLASSES)
            floor = max(1.0 / (counts[c] * (n_part - counts[c])) for c in cls)
            tol = max(4.0 * g["auroc_diff"][key], floor)
            print(f"\n{cfg} {key}: {metrics[key]:.8f} vs {want:.8f} (tolerance {tol:.2e})")
            assert abs(metrics[key] - want) <= tol, key


def test_pipeline_takes_a_device_tensor_and_transforms_like_its_parts():
    from viscy_amd.linear_classifier import train_linear_classifier

    x = RL.pipe_arrays()[0]
    pipe, metrics, val = device_pipeline("scaled_pca8")
    ad = RL.pipe_adata(torch.from_numpy(x.copy()).to(DEV))
    pipe2, metrics2, val2 = train_linear_classifier(ad, RL.pipe_task(), use_scaling=True, use_pca=True, n_pca_components=8,
                                                    classifier_params=dict(RL.PIPE_PARAMS), split_train_data=0.8, random_seed=42)
    assert metrics2 == metrics and np.array_equal(val2["y_val_proba"], val["y_val_proba"])
    t = pipe.transform(x)
    assert isinstance(t, np.ndarray) and t.dtype == np.float32 and t.shape == (600, 8)
    assert np.array_equal(pipe.predict(x[:50]), pipe.classifier.predict(t[:50]))
    assert np.array_equal(pipe.predict_proba(x[3:4]), pipe.predict_proba(x[:50])[3:4])        # a single row


def test_predict_with_classifier_writes_the_references_keys():
    from viscy_amd.linear_classifier import predict_with_classifier

    g = golden()["predict"]
    pipe = device_pipeline("scaled_all")[0]
    task = RL.pipe_task()
    meta = {"artifact_name": "m:v3", "artifact_id": "id7", "artifact_version": "v3"}
    ad = predict_with_classifier(RL.pipe_adata(), pipe, task, artifact_metadata=meta, include_wells=["A/1", "B/2"])
    assert sorted(ad.obs.columns) == g["obs_keys"] and sorted(ad.obsm) == g["obsm_keys"] and ad.uns == g["uns"]
    pred = ad.obs[f"predicted_{task}"]
    nan_rows = np.flatnonzero(pred.isna().to_numpy())
    assert np.array_equal(nan_rows, g["nan_rows"].numpy()) and 0 < len(nan_rows) < len(pred)
    proba = ad.obsm[f"predicted_{task}_proba"]
    assert proba.shape == (600, 3) and np.isnan(proba[nan_rows]).all() and np.isfinite(np.delete(proba, nan_rows, axis=0)).all()
    assert [p if isinstance(p, str) else None for p in pred] == g["pred"]      # every row of the fixture is decided
    everyone = predict_with_classifier(RL.pipe_adata(), pipe, task)
    assert not everyone.obs[f"predicted_{task}"].isna().any() and f"classifier_{task}_id" not in everyone.uns
