"""CPU: the yardsticks of the test-stage tests and the host layer of the test stage.

The float64 restatements of tests/ref_test_metrics.py against scipy / sklearn / numpy; ``viscy_amd.metrics.metrics_from_sums`` on
exact sums; the "windows inside the image" statement of SSIM against both padded readings of the library; the tap tables; the
golden ``ssim_25d`` / ``ms_ssim_25d`` values against the oracle's restatement; ``Trainer.test`` (hook order, batch-size weighting,
``on_epoch=False`` keys) on stub modules; the ``test`` subcommand; the argument checks of the metric functions; ``VSUNet.test_step``
on the CPU plumbing model."""

import json
import math

import numpy as np
import pytest
import torch

from tests import ref_test_metrics as R
from tests.conftest import load_golden


def _pair(shape, offset, seed):
    rng = np.random.default_rng(seed)
    t = (rng.normal(size=shape) + offset).astype(np.float32)
    return (t + 0.3 * rng.normal(size=shape)).astype(np.float32), t


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_regression_restatement_matches_scipy_sklearn_numpy(offset):
    from scipy.stats import pearsonr
    from sklearn.metrics import mean_absolute_error, mean_squared_error, r2_score

    p, t = _pair((2, 33, 47), offset, 1)
    got = R.regression64(p, t)
    p64, t64 = p.astype(np.float64).ravel(), t.astype(np.float64).ravel()
    n = p.size
    tol = 4 * n * R.U64  # two float64 statements of one well-conditioned (centred) quantity over n terms
    assert abs(got["MAE"] - mean_absolute_error(t64, p64)) <= tol * got["MAE"]
    assert abs(got["MSE"] - mean_squared_error(t64, p64)) <= tol * got["MSE"]
    assert abs(got["pearson"] - pearsonr(p64, t64)[0]) <= tol
    assert abs(got["r2"] - r2_score(t64, p64)) <= tol
    rows_p, rows_t = p.astype(np.float64).reshape(-1, p.shape[-1]), t.astype(np.float64).reshape(-1, p.shape[-1])
    cos = np.mean([np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)) for a, b in zip(rows_p, rows_t)])
    assert abs(got["cosine"] - cos) <= tol
    want = torch.nn.functional.cosine_similarity(torch.from_numpy(rows_p), torch.from_numpy(rows_t), dim=-1).mean().item()
    assert abs(got["cosine"] - want) <= tol


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_metrics_from_sums_on_exact_sums(offset):
    from viscy_amd.metrics import SUM_NAMES, metrics_from_sums

    assert len(SUM_NAMES) == R.NQ == 13
    p, t = _pair((3, 20, 31), offset, 2)
    s, mag = R.exact_sums(p, t)
    # numpy's own float64 sums agree with the fsum statement to their pairwise rounding
    assert abs(s[4] - (p.astype(np.float64) * t.astype(np.float64)).sum()) <= 64 * R.U64 * mag[4]
    got, want = metrics_from_sums(s, p.size), R.regression64(p, t)
    bound = R.metric_bounds(s, np.zeros(R.NQ), p.size)  # the host arithmetic's share alone
    for k, v in want.items():
        assert isinstance(got[k], float)
        assert abs(got[k] - v) <= bound[k] + 4 * p.size * R.U64 * max(1.0, abs(v)), (k, got[k], v, bound[k])
    # the same arithmetic on a float64 tensor stays a tensor
    tens = metrics_from_sums(torch.from_numpy(s), p.size)
    assert all(torch.is_tensor(v) and v.dtype == torch.float64 and v.ndim == 0 for v in tens.values())
    assert all(abs(tens[k].item() - got[k]) <= 4 * R.U64 * max(1.0, abs(got[k])) for k in got)


def test_metrics_from_sums_constant_input_is_nan_where_the_definition_is():
    from viscy_amd.metrics import metrics_from_sums

    p = np.full((1, 4, 8), 2.0, dtype=np.float32)
    t = np.full((1, 4, 8), 3.0, dtype=np.float32)
    s, _ = R.exact_sums(p, t)
    m = metrics_from_sums(s, p.size)
    assert m["MAE"] == 1.0 and m["MSE"] == 1.0 and abs(m["cosine"] - 1.0) <= 4 * R.U64
    assert math.isnan(m["pearson"])  # 0 / 0
    assert m["r2"] == -math.inf      # 1 - 32 / 0
    s, _ = R.exact_sums(p, p)
    m = metrics_from_sums(s, p.size)
    assert math.isnan(m["pearson"]) and math.isnan(m["r2"])
    mt = metrics_from_sums(torch.from_numpy(s), p.size)
    assert bool(torch.isnan(mt["pearson"])) and bool(torch.isnan(mt["r2"]))


def test_metric_bounds_grow_with_the_sums_bounds_and_refuse_constant_data():
    p, t = _pair((1, 8, 16), 1000.0, 3)
    s, mag = R.exact_sums(p, t)
    e = R.sum_bounds(p[None][0].reshape(1, 8, 16), t.reshape(1, 8, 16), s, mag)
    assert (e[[7, 8, 9, 10, 12]] == 0).all() and (e[[0, 1, 2, 3, 4, 5, 6, 11]] > 0).all()
    b0, b1 = R.metric_bounds(s, np.zeros(R.NQ), p.size), R.metric_bounds(s, e, p.size)
    assert all(b1[k] > b0[k] > 0 for k in b0)
    const = np.full((1, 8, 16), 5.0, dtype=np.float32)
    sc, _ = R.exact_sums(const, const)
    with pytest.raises(AssertionError, match="constant"):
        R.metric_bounds(sc, np.zeros(R.NQ), const.size)


def test_launch_constants_and_depths():
    from viscy_amd import _lib as L

    assert (L.PAIR_SUMS, L.PAIR_SUMS_WAVES, L.PAIR_SUMS_VEC, L.SSIM_MAX_K) == (13, 4, 4, 33) and L.SSIM_TILE >= 8
    assert R.pair_launch(1, 1) == (1, 1) and R.pair_launch(1, 4 * L.PAIR_SUMS_MAX_WGS + 1) == (L.PAIR_SUMS_MAX_WGS, 2)
    d_small, row_small = R.pair_depth(1, 1, 1)
    d_big, row_big = R.pair_depth(8, 2048, 2048)
    assert row_small == 5 + 6 and row_big == 4 * 8 + 1 + 6 and d_big > d_small
    names = [c["name"] for c in R.pair_cases()]
    assert len(set(names)) == len(names)
    assert any(c["planes"] * c["H"] > L.PAIR_SUMS_WAVES * L.PAIR_SUMS_MAX_WGS for c in R.pair_cases())  # rows past one launch's waves
    assert any(c["ps"] % 4 for c in R.pair_cases()) and any(c["rs"] > c["W"] for c in R.pair_cases())
    ts = L.SSIM_TILE
    extents = {e for c in R.ssim_exact_cases() for e in (c["H"] - c["Ky"] + 1, c["W"] - c["Kx"] + 1)}
    assert {1, ts - 1, ts, ts + 1, 2 * ts + 1} <= extents
    assert {c["Ky"] for c in R.ssim_exact_cases()} >= {3, 11, 21, 33}
    assert any(c["Ky"] != c["Kx"] and c["H"] != c["W"] for c in R.ssim_exact_cases())


def test_valid_windows_equal_both_padded_readings():
    """reflect pad 10 / crop 10 (the newer library) and pad 5 / crop 5 (the older one: the pad of the Gaussian size) leave exactly
    the windows that never touch the padding: the same numbers, to the last bit, as the windows inside the image"""
    g = torch.Generator().manual_seed(4)
    t = torch.rand((2, 47, 53), generator=g, dtype=torch.float64) * 3 + 10
    p = t + 0.3 * torch.randn(t.shape, generator=g, dtype=torch.float64)
    K = 21
    taps = np.full(K, 1.0 / K)
    c1, c2 = (0.01 * 4.0) ** 2, (0.03 * 4.0) ** 2
    w = torch.full((1, 1, K, K), 1.0 / (K * K), dtype=torch.float64)
    # the padded routes and the unpadded one with the same arithmetic (no centring): bit-equal
    P, T = p[:, None], t[:, None]
    mp, mt, epp, ett, ept = [torch.nn.functional.conv2d(v, w) for v in (P, T, P * P, T * T, P * T)]
    plain = (((2 * mp * mt + c1) * (2 * (ept - mp * mt) + c2)) /
             ((mp * mp + mt * mt + c1) * ((epp - mp * mp).clamp_min(0) + (ett - mt * mt).clamp_min(0) + c2)))[:, 0]
    assert plain.shape == (2, 47 - K + 1, 53 - K + 1)
    for pad in (10, 5):
        padded = R.ssim_padded64(p, t, K, pad, c1, c2)
        assert padded.shape == plain.shape
        assert float((padded - plain).abs().max()) == 0.0, pad
    # and the centred statement the tests use is the same quantity
    centred = R.ssim_valid64(p, t, taps, taps, c1, c2)
    assert float((centred - plain).abs().max()) <= 1e-12


def test_fp32_library_statement_loses_the_offset_and_the_centred_one_does_not():
    """the reason the kernel centres before it squares: the yardstick's own error explodes with the offset"""
    case = {"name": "u21", "kind": "uniform", "K": 21, "H": 64, "W": 64}
    taps = R.real_taps(case)
    errs = {}
    for off in (0.0, 1000.0):
        p, t = R.real_images(case, off)
        c1, c2 = R.c_of(max(float(p.max() - p.min()), float(t.max() - t.min())))
        want = R.ssim_valid64(p, t, taps, taps, c1, c2)
        errs[off] = float((R.ssim_library_fp32(p, t, taps, taps, c1, c2).double() - want).abs().max())
    assert errs[0.0] < 1e-4 and errs[1000.0] > 100 * errs[0.0], errs
    fx = R.real_fixture(case)
    assert fx["yard_max"] == errs[0.0] and fx["yard_mean"] <= fx["yard_max"]
    R.clear_fixtures()


def test_ssim_bound_covers_an_fp32_evaluation_of_the_formula():
    """the running bound of ssim_formula64 against the formula evaluated in fp32 numpy (one rounding per operation, as the kernel)"""
    case = R.ssim_exact_cases()[3]
    p, t = R.integer_images(case)
    wy, wx = R.dyadic_taps(case["Ky"]), R.dyadic_taps(case["Kx"], phase=1)
    f = np.float32
    seen = []
    for sp, st in R.EXACT_SHIFTS:
        means = [m.numpy() for m in R.window_means64(p, t, wy, wx, sp, st)]
        assert all((m.astype(f).astype(np.float64) == m).all() for m in means)  # exact in fp32
        mx, my, exx, eyy, exy = [m.astype(f) for m in means]
        c1, c2 = f(R.EXACT_C[0]), f(R.EXACT_C[1])
        vxx, vyy, vxy = np.maximum(exx - mx * mx, f(0)), np.maximum(eyy - my * my, f(0)), exy - mx * my
        mp, mt = mx + f(sp), my + f(st)
        got = ((f(2) * (mp * mt) + c1) * (f(2) * vxy + c2)) / (((mp * mp + mt * mt) + c1) * ((vxx + vyy) + c2))
        assert got.dtype == np.float32
        want, bound = R.ssim_valid64(p, t, wy, wx, *R.EXACT_C, with_bound=True, sp=sp, st=st)
        ratio = float((np.abs(got.astype(np.float64) - want.numpy()) / bound.numpy()).max())
        assert 0 < ratio <= 1.0, ratio
        assert float(bound.max()) < 1e-3
        seen.append((torch.from_numpy(got.astype(np.float64)), bound))
    (m0, b0), (m1, b1) = seen  # integer shifts keep the centred values exact: two evaluations of one value
    assert bool(((m0 - m1).abs() <= b0 + b1).all())


def test_tap_tables():
    from viscy_amd.metrics import gaussian_window_size, window_taps

    u = window_taps(21)
    assert u.dtype == np.float32 and u.shape == (21,) and (u == np.float32(1.0) / np.float32(21)).all()
    assert gaussian_window_size(1.5) == 11 and gaussian_window_size(0.5) == 5 and gaussian_window_size(2.5) == 19
    g = window_taps(11, 1.5)
    d = np.arange(-5, 6, dtype=np.float64)
    want = np.exp(-(d / 1.5) ** 2 / 2)
    want /= want.sum()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert np.abs(g - want).max() <= 8 * R.U32 * want.max()  # an exp, a square, a division and an 11-term sum in fp32
    assert (g == g[::-1]).all() and abs(float(g.astype(np.float64).sum()) - 1.0) <= 11 * R.U32
    for k in (3, 11, 21, 33):
        taps = R.dyadic_taps(k)
        assert all(math.log2(v).is_integer() for v in taps) and float(taps.astype(np.float64).sum()) == 1.0
        assert (R.dyadic_taps(k, phase=1) != taps).any()


def test_golden_ms_ssim_values_are_what_the_oracle_restates():
    """the fixture itself: the reference's results against oracle/loss_ref.py on the stacks rebuilt from the seeds"""
    from oracle import loss_ref

    gold = load_golden(R.GOLDEN_FILE)["cases"]
    assert set(gold) == set(R.GOLDEN_CASES)
    for name, case in R.GOLDEN_CASES.items():
        rec = gold[name]
        assert tuple(rec["shape"]) == tuple(case["shape"]) and rec["seed"] == case["seed"]
        pred, target = R.golden_stacks(name)
        ssim, cs = loss_ref.ssim_25d(pred, target)
        torch.testing.assert_close(ssim, rec["ssim"][0], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(cs, rec["ssim"][1], rtol=1e-5, atol=1e-6)
        assert rec["ssim"][0].shape == (case["shape"][0],)
        for key, _, kw in R.golden_calls(name)[1:]:
            want = loss_ref.ms_ssim_25d(pred, target, **kw)
            assert rec[key].ndim == 0 and rec[key].item() > 0
            torch.testing.assert_close(want, rec[key], rtol=1e-5, atol=1e-6)
        assert rec["ms_ssim_clamp"].item() != rec["ms_ssim_clamp_betas3"].item()
    # on the anti-correlated stacks the clamp is what is measured: without it a negative number meets a fractional power
    pred, target = R.golden_stacks("anti_d1_176")
    assert not bool(torch.isfinite(loss_ref.ms_ssim_25d(pred, target, clamp=False)))
    assert bool((gold["anti_d1_176"]["ssim"][1] < 0).all())


# ------------------------------------------------------------------------------------------------ Trainer.test
class _StubModule(torch.nn.Module):
    def __init__(self, events):
        super().__init__()
        self.events, self.logged, self.logged_kw = events, {}, {}

    def _log(self, key, value, **kw):
        self.logged.setdefault(key, []).append(value)
        self.logged_kw[key] = kw

    def on_test_start(self):
        self.events.append("module.on_test_start")

    def on_test_epoch_end(self):
        self.events.append("module.on_test_epoch_end")

    def on_test_end(self):
        self.events.append("module.on_test_end")

    def test_step(self, batch, batch_idx):
        assert not self.training and not torch.is_grad_enabled()
        self.events.append(f"test_step {batch_idx}")
        x = batch["source"]
        assert batch["seen_by_transfer"] == batch_idx
        self._log("m/mean", x.mean(), on_step=True, on_epoch=True)
        self._log("m/default", x.double().sum() / x.shape[0])               # Lightning's default in a test step: on_epoch
        self._log("m/own_weight", torch.tensor(float(batch_idx)), on_epoch=True, batch_size=1)
        self._log("position", torch.tensor(float(batch_idx)), on_step=True, on_epoch=False)
        return {"m/mean": x.mean()}


class _StubData:
    def __init__(self, events, batches):
        self.events, self.batches, self.training = events, batches, True

    def setup(self, stage):
        self.events.append(f"setup {stage}")

    def test_dataloader(self):
        return [dict(b) for b in self.batches]

    def on_after_batch_transfer(self, batch, dataloader_idx):
        assert self.training is False
        last_setup = len(self.events) - 1 - self.events[::-1].index("setup test")
        batch["seen_by_transfer"] = self.events[last_setup:].count("transfer")
        self.events.append("transfer")
        return batch


class _StubCallback:
    def __init__(self, events):
        self.events = events

    def on_test_start(self, trainer, module):
        assert trainer.testing
        self.events.append("cb.on_test_start")

    def on_test_batch_end(self, trainer, module, outputs, batch, batch_idx, dataloader_idx):
        assert "m/mean" in outputs and dataloader_idx == 0
        self.events.append(f"cb.on_test_batch_end {batch_idx}")

    def on_test_epoch_end(self, trainer, module):
        self.events.append("cb.on_test_epoch_end")

    def on_test_end(self, trainer, module):
        self.events.append("cb.on_test_end")


def test_trainer_test_loop_on_stubs(monkeypatch):
    from viscy_amd.trainer import Trainer

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    events = []
    a = torch.arange(3 * 4, dtype=torch.float32).reshape(3, 4)   # batch of 3, mean 5.5
    b = torch.full((1, 4), 100.0)                                # batch of 1, mean 100
    module, data = _StubModule(events), _StubData(events, [{"source": a}, {"source": b}])
    trainer = Trainer(callbacks=[_StubCallback(events)])
    module.train()
    out = trainer.test(module, data)
    first = list(events)
    assert first == ["setup test", "cb.on_test_start", "module.on_test_start", "transfer", "test_step 0", "cb.on_test_batch_end 0",
                      "transfer", "test_step 1", "cb.on_test_batch_end 1", "cb.on_test_epoch_end", "module.on_test_epoch_end",
                      "cb.on_test_end", "module.on_test_end"]
    assert isinstance(out, list) and len(out) == 1 and set(out[0]) == {"m/mean", "m/default", "m/own_weight"}  # no on_epoch=False key
    assert all(isinstance(v, float) for v in out[0].values())
    assert out[0]["m/mean"] == (3 * 5.5 + 1 * 100.0) / 4          # weighted by batch size, not the mean of the two means
    assert out[0]["m/default"] == (3 * 22.0 + 1 * 400.0) / 4
    assert out[0]["m/own_weight"] == 0.5                          # an explicit batch_size is the weight
    assert module.logged["position"] == [torch.tensor(0.0), torch.tensor(1.0)]
    assert trainer.testing is False and data.training is True and trainer.datamodule is data and module.trainer is trainer
    # a second epoch starts from nothing: the earlier values in module.logged are not counted again
    assert trainer.test(module, data) == out


def test_trainer_test_refuses_more_than_one_rank(monkeypatch):
    import torch.distributed as dist

    from viscy_amd.trainer import Trainer

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    events = []
    with pytest.raises(NotImplementedError, match="world size 2"):
        Trainer().test(_StubModule(events), _StubData(events, []))
    assert events == []


def test_cli_test_subcommand(monkeypatch, capsys):
    from viscy_amd import config

    args = config.parser().parse_args(["test", "-c", "a.yml", "--config", "b.yml"])
    assert args.subcommand == "test" and args.config == ["a.yml", "b.yml"]
    with pytest.raises(SystemExit):
        config.parser().parse_args(["test"])          # --config is required
    with pytest.raises(SystemExit):
        config.parser().parse_args(["evaluate", "-c", "a.yml"])
    calls = []

    class _T:
        def test(self, module, datamodule):
            calls.append((module, datamodule))
            return [{"test_metrics/MAE": 0.25, "test_metrics/SSIM": 0.5}]

    monkeypatch.setattr(config, "load_composed_config", lambda path: {"model": path})
    monkeypatch.setattr(config, "build", lambda cfg: ("module", "data", _T(), []))
    assert config.main(["test", "--config", "x.yml"]) == 0
    assert calls == [("module", "data")]
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == {"test_metrics/MAE": 0.25, "test_metrics/SSIM": 0.5}


# ------------------------------------------------------------------------------------------------ argument checks, CPU plumbing model
def test_metric_functions_refuse_what_is_not_built(monkeypatch):
    from viscy_amd import metrics as M

    x4, x5 = torch.zeros(1, 1, 40, 40), torch.zeros(1, 1, 1, 40, 40)
    with pytest.raises(NotImplementedError, match="preds"):
        M.structural_similarity_index_measure(x5, x5)
    with pytest.raises(ValueError, match="kernel_size"):
        M.structural_similarity_index_measure(x4, x4, gaussian_kernel=False, kernel_size=20)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        M.structural_similarity_index_measure(x4, x4, gaussian_kernel=False, kernel_size=35)
    with pytest.raises(NotImplementedError, match="sigma"):
        M.structural_similarity_index_measure(x4, x4, sigma=5.0)
    with pytest.raises(NotImplementedError, match="data_range"):
        M.structural_similarity_index_measure(x4, x4, data_range=(0.0, 1.0))
    with pytest.raises(ValueError, match="reduction"):
        M.structural_similarity_index_measure(x4, x4, reduction="mean")
    with pytest.raises(NotImplementedError, match="in_plane_window_size"):
        M.ssim_25d(x5, x5, in_plane_window_size=(7, 7))
    with pytest.raises(NotImplementedError, match="in_plane_window_size"):
        M.ms_ssim_25d(x5, x5, in_plane_window_size=(11, 7))
    with pytest.raises(ValueError, match="Input shape"):
        M.ssim_25d(x4, x4)
    with pytest.raises(NotImplementedError, match="reduction"):
        M.cosine_similarity(x4, x4, reduction="sum")
    # no CPU path: without a HIP device every entry point says so
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for fn in (M.regression_metrics, M.mean_absolute_error, M.pearson_corrcoef, M.r2_score, M.mean_squared_error, M.cosine_similarity):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x4, x4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.structural_similarity_index_measure(x4, x4, gaussian_kernel=False, kernel_size=21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.ms_ssim_25d(torch.zeros(1, 1, 1, 176, 176), torch.zeros(1, 1, 1, 176, 176))


def test_metrics_module_imports_no_test_or_oracle_code():
    import ast
    import inspect

    from viscy_amd import metrics as M

    tree = ast.parse(inspect.getsource(M))
    names = [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)] + \
            [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert not [n for n in names if n.split(".")[0] in ("oracle", "tests", "torchmetrics")], names


def test_planes_reads_views_in_place():
    from viscy_amd.metrics import _planes

    cpu = torch.device("cpu")
    x = torch.zeros(2, 2, 5, 24, 40)
    v, planes, H, W, ps, rs = _planes(x[:, 0, 2:3], cpu, "x")
    assert v.data_ptr() == x[0, 0, 2].data_ptr() and (planes, H, W, ps, rs) == (2, 24, 40, 2 * 5 * 24 * 40, 40)
    v, planes, H, W, ps, rs = _planes(x[..., 3:20, 5:30], cpu, "x")           # leading axes fold, rows keep their stride
    assert v.data_ptr() == x[0, 0, 0, 3, 5:].data_ptr() and (planes, H, W, ps, rs) == (20, 17, 25, 24 * 40, 40)
    v, planes, H, W, ps, rs = _planes(x[:, :, ::2], cpu, "x")                 # (2, 2, 3, ...) with strides that do not fold: a copy
    assert v.is_contiguous() and (planes, H, W, ps, rs) == (12, 24, 40, 24 * 40, 40)
    v, planes, H, W, ps, rs = _planes(x[..., ::2], cpu, "x")                  # X stride 2: a copy
    assert v.is_contiguous() and (planes, W, rs) == (20, 20, 20)
    v, planes, H, W, ps, rs = _planes(torch.zeros(7, 9), cpu, "x")
    assert (planes, H, W, ps, rs) == (1, 7, 9, 0, 9)
    with pytest.raises(ValueError, match="two axes"):
        _planes(torch.zeros(7), cpu, "x")


def test_test_step_on_the_cpu_model_is_what_it_was(monkeypatch):
    """the "2D" plumbing model on CPU tensors: the five keys by the plain tensor arithmetic, no SSIM key, the index keys"""
    from viscy_amd.vsunet import VSUNet

    torch.manual_seed(0)
    m = VSUNet(architecture="2D", model_config=dict(in_channels=1, out_channels=1, num_blocks=2, num_filters=(4, 8, 16), task="reg")).eval()
    g = torch.Generator().manual_seed(1)
    batch = {"source": torch.randn(2, 1, 1, 32, 32, generator=g), "target": torch.randn(2, 1, 1, 32, 32, generator=g),
             "index": (["plate/A/1/3/0", "plate/A/1/4/0"], torch.tensor([2, 0]), torch.tensor([7, 1]))}
    with torch.no_grad():
        mets = m.test_step(batch, 0)
        pred = m(batch["source"])
    assert set(mets) == {f"test_metrics/{k}" for k in ("MAE", "MSE", "cosine", "pearson", "r2")}
    want = R.regression64(pred[:, 0, 0:1].numpy(), batch["target"][:, 0, 0:1].numpy())
    for k, v in want.items():
        assert abs(mets[f"test_metrics/{k}"].item() - v) <= 1e-5 * max(1.0, abs(v)), k  # fp32 tensor arithmetic on 2048 values
    assert m.logged_kw["test_metrics/MAE"] == {"on_step": True, "on_epoch": True}
    assert m.logged_kw["position"]["on_epoch"] is False
    assert [v.item() for v in (m.logged["position"][0], m.logged["time"][0], m.logged["slice"][0])] == [3.0, 2.0, 7.0]
    assert "test_metrics/SSIM" not in m.logged
