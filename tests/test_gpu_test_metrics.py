"""GPU: the test-stage kernels (csrc/test_metrics.hip), their Python layer (viscy_amd/metrics.py) and the test stage end to end.

vsx_pair_sums: integer images bit-equal to int64 arithmetic at every launch edge (tests/ref_test_metrics.py: pair_cases), inputs
inside NaN-poisoned buffers, two runs bit-identical; real-valued images at offsets 0 and 1000 within the counted float64 bound, also
after metrics_from_sums.  vsx_ssim_window: dyadic taps on integer images (exact window means) within the counted fp32 bound of the
formula, the plane sums within the fold bound of the kernel's own map, P == T exactly 1, real-valued images at offsets 0 / 100 /
1000 within twice the fp32 library statement's own error at offset 0, refusals that launch nothing.  The functional metrics, SSIM
and ssim_25d / ms_ssim_25d against the float64 statements and the reference's golden values; Trainer.test on a tiny UNeXt2.
The worst observed ratios are in profiles/test_metrics_margins.txt."""

import pytest
import torch

from tests import ref_test_metrics as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _env():
    from viscy_amd import _lib

    return R.LibEntry(_lib.lib()), torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    R.clear_fixtures()
    torch.cuda.empty_cache()


def _ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------ vsx_pair_sums
@pytest.mark.parametrize("case", R.pair_cases(), ids=_ids(R.pair_cases()))
def test_pair_sums_integer_images_are_bit_exact(case):
    ep, dev = _env()
    R.run_pair_exact(ep, case, dev)


@pytest.mark.parametrize("case", R.real_pair_cases(), ids=_ids(R.real_pair_cases()))
def test_pair_sums_real_images_within_the_counted_bound(case):
    ep, dev = _env()
    R.run_pair_real(ep, case, dev)


def test_pair_sums_cosine_of_zero_and_equal_rows():
    """a zero row has cosine 0 (0 / (1e-8 * 1e-8)); a row of equal images has cosine 1 within the counted bound"""
    ep, dev = _env()
    case = R._pc("cosine_rows", 1, 4, 70)
    g = torch.Generator().manual_seed(1)
    p = torch.randn((1, 4, 70), generator=g)
    t = p.clone()
    p[0, 1] = 0.0                     # row 1: prediction zero
    t[0, 2] = 0.0                     # row 2: target zero
    p[0, 3], t[0, 3] = 0.0, 0.0       # row 3: both
    got = ep.pair_sums(R.Poisoned(p, case, dev), R.Poisoned(t, case, dev), case, dev)
    s, mag = R.exact_sums(p.numpy(), t.numpy())
    e = R.sum_bounds(p.numpy(), t.numpy(), s, mag)
    assert abs(s[11] - 1.0) <= 4 * R.U64             # the statement itself: 1 + 0 + 0 + 0
    assert abs(got[11].item() - 1.0) <= e[11] and got[12].item() == 4.0, (got[11].item(), e[11])
    zero = torch.zeros((1, 4, 70))
    got = ep.pair_sums(R.Poisoned(zero, case, dev), R.Poisoned(zero, case, dev), case, dev)
    assert got[11].item() == 0.0 and got[2].item() == 0.0


# ------------------------------------------------------------------------------------------------ vsx_ssim_window
@pytest.mark.parametrize("case", R.ssim_exact_cases(), ids=_ids(R.ssim_exact_cases()))
def test_ssim_window_exact_means_within_the_counted_bound(case):
    ep, dev = _env()
    R.run_ssim_exact(ep, case, dev)


@pytest.mark.parametrize("case", R.ssim_exact_cases()[1::3], ids=_ids(R.ssim_exact_cases()[1::3]))
def test_ssim_window_of_identical_images_is_exactly_one(case):
    ep, dev = _env()
    R.run_ssim_identical(ep, case, dev)


@pytest.mark.parametrize("case", R.ssim_real_cases(), ids=_ids(R.ssim_real_cases()))
def test_ssim_window_real_images_within_twice_the_fp32_library_error(case):
    """measured (profiles/test_metrics_margins.txt): map error 0.05 - 0.12 of the yardstick at every offset, mean error at most
    0.65 of it; the factor 2 is not widened"""
    ep, dev = _env()
    R.run_ssim_real(ep, case, dev)


def test_refused_arguments_launch_nothing():
    ep, dev = _env()
    R.run_ssim_refusals(ep, dev)


# ------------------------------------------------------------------------------------------------ Python layer
def _numpy_metrics(p: torch.Tensor, t: torch.Tensor):
    from viscy_amd.metrics import metrics_from_sums

    p3, t3 = p.reshape(-1, *p.shape[-2:]).numpy(), t.reshape(-1, *t.shape[-2:]).numpy()
    s, mag = R.exact_sums(p3, t3)
    e = R.sum_bounds(p3, t3, s, mag)
    return metrics_from_sums(s, p.numel()), R.metric_bounds(s, e, p.numel())


def test_functional_metrics_match_metrics_from_sums_of_exact_sums():
    from viscy_amd import metrics as M

    g = torch.Generator().manual_seed(6)
    full_t = torch.randn((2, 2, 5, 24, 40), generator=g) + 1000.0
    full_p = full_t + 0.3 * torch.randn(full_t.shape, generator=g)
    dp, dt = full_p.cuda(), full_t.cuda()
    vp, vt = dp[:, 0, 2:3], dt[:, 0, 2:3]                      # what test_step passes: read in place
    want, bound = _numpy_metrics(full_p[:, 0, 2:3].contiguous(), full_t[:, 0, 2:3].contiguous())
    got = M.regression_metrics(vp, vt)
    assert set(got) == {"MAE", "MSE", "cosine", "pearson", "r2"}
    single = {"MAE": M.mean_absolute_error, "MSE": M.mean_squared_error, "cosine": M.cosine_similarity, "pearson": M.pearson_corrcoef,
              "r2": M.r2_score}
    for k, v in want.items():
        assert got[k].dtype == torch.float64 and got[k].is_cuda and got[k].ndim == 0
        assert abs(got[k].item() - v) <= bound[k], (k, got[k].item(), v, bound[k])
        assert single[k](vp, vt).item() == got[k].item(), k       # the same launch, the same bits
    # a numpy pair is uploaded; sums come back under their names
    s = M.pair_sums(full_p[0, 0].numpy(), full_t[0, 0].numpy())
    assert s.shape == (len(M.SUM_NAMES),) and s[12].item() == 5 * 24
    assert s[7].item() == float(full_p[0, 0].min()) and s[10].item() == float(full_t[0, 0].max())


def _ssim_want(p, t, taps, data_range, shape_bc):
    dr = data_range if data_range is not None else max(float(p.max() - p.min()), float(t.max() - t.min()))
    c1, c2 = R.c_of(dr)
    m = R.ssim_valid64(p.reshape(-1, *p.shape[-2:]), t.reshape(-1, *t.shape[-2:]), taps, taps, c1, c2)
    lib32 = R.ssim_library_fp32(p.reshape(-1, *p.shape[-2:]), t.reshape(-1, *t.shape[-2:]), taps, taps, c1, c2).double()
    return m.view(*shape_bc, *m.shape[-2:]), float((lib32 - m).abs().max())


@pytest.mark.parametrize("gaussian", [False, True], ids=["uniform21", "gaussian11"])
@pytest.mark.parametrize("data_range", [None, 5.0], ids=["range_from_data", "range_given"])
def test_structural_similarity_matches_the_float64_statement(gaussian, data_range):
    """a map value is allowed twice the fp32 library statement's own error on these images (the bound the kernel test holds the
    map to); a mean of map values cannot be further off than the worst of them"""
    from viscy_amd import metrics as M

    g = torch.Generator().manual_seed(8)
    t = torch.rand((2, 3, 70, 83), generator=g) * 3
    p = t + 0.3 * torch.randn(t.shape, generator=g)
    taps = M.window_taps(11, 1.5) if gaussian else M.window_taps(21)
    want, yard = _ssim_want(p, t, taps, data_range, (2, 3))
    tol = 2 * yard
    kw = dict(gaussian_kernel=True, sigma=1.5) if gaussian else dict(gaussian_kernel=False, kernel_size=21)
    per_sample = want.mean((1, 2, 3))
    val, full = M.structural_similarity_index_measure(p.cuda(), t.cuda(), data_range=data_range, return_full_image=True, **kw)
    assert full.shape == want.shape and full.dtype == torch.float32
    assert float((full.cpu().double() - want).abs().max()) <= tol
    assert val.ndim == 0 and abs(val.item() - per_sample.mean().item()) <= tol
    s = M.structural_similarity_index_measure(p.cuda(), t.cuda(), data_range=data_range, reduction="sum", **kw)
    assert abs(s.item() - per_sample.sum().item()) <= 2 * tol
    for red in ("none", None):
        n = M.structural_similarity_index_measure(p.cuda(), t.cuda(), data_range=data_range, reduction=red, **kw)
        assert n.shape == (2,) and float((n.cpu() - per_sample).abs().max()) <= tol
    # views are read in place and give the same bits as their copies
    big_p, big_t = torch.zeros(2, 3, 80, 90).cuda(), torch.zeros(2, 3, 80, 90).cuda()
    big_p[..., 4:74, 5:88], big_t[..., 4:74, 5:88] = p.cuda(), t.cuda()
    v = M.structural_similarity_index_measure(big_p[..., 4:74, 5:88], big_t[..., 4:74, 5:88], data_range=data_range, **kw)
    assert v.item() == val.item()


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_ssim_25d_and_ms_ssim_25d_match_the_reference_golden(name):
    """tolerance: what test_gpu_model.py::test_mixed_loss_vs_reference_golden allows (1e-3 relative)"""
    from viscy_amd import metrics as M

    rec = load_golden(R.GOLDEN_FILE)["cases"][name]
    pred, target = R.golden_stacks(name)
    p, t = pred.cuda(), target.cuda()
    fns = {"ssim_25d": M.ssim_25d, "ms_ssim_25d": M.ms_ssim_25d}
    for key, fn, kw in R.golden_calls(name):
        got = fns[fn](p, t, **kw)
        got, want = (got, rec[key]) if isinstance(got, tuple) else ((got,), (rec[key],))
        for a, b in zip(got, want):
            assert a.shape == b.shape, (key, a.shape, b.shape)
            assert bool(((a.cpu().double() - b.double()).abs() <= R.GOLDEN_RTOL * b.double().abs()).all()), (name, key, a, b)
    assert M.ssim_25d(p, t).shape == (pred.shape[0],)
    if R.GOLDEN_CASES[name].get("anti"):
        assert not bool(torch.isfinite(M.ms_ssim_25d(p, t)))     # clamp=False is the default, as in the reference
    with pytest.raises(ValueError, match="176"):
        M.ms_ssim_25d(p[..., :175], t[..., :175])


# ------------------------------------------------------------------------------------------------ end to end
class _ListData:
    """a datamodule over ready batches"""

    def __init__(self, batches):
        self.batches, self.training = batches, False

    def setup(self, stage):
        assert stage == "test"

    def test_dataloader(self):
        return [dict(b) for b in self.batches]

    def on_after_batch_transfer(self, batch, dataloader_idx):
        return batch


def test_trainer_test_end_to_end_on_a_tiny_unext2():
    from viscy_amd import metrics as M
    from viscy_amd.trainer import Trainer
    from viscy_amd.vsunet import VSUNet

    torch.manual_seed(0)
    # the tiny backbone in the trainer's default precision (bf16): its forward without a backward is bit-reproducible, which the
    # fp32 kernels that convnextv2_atto falls back to (60 decoder channels) are not
    kw = dict(in_channels=1, out_channels=2, in_stack_depth=5, backbone="convnextv2_tiny", head_pool=True)
    module = VSUNet(architecture="UNeXt2", model_config=kw)
    g = torch.Generator().manual_seed(3)
    batches = []
    for b, pos in ((2, "7"), (1, "8")):
        batches.append({"source": torch.randn((b, 1, 5, 64, 64), generator=g), "target": torch.rand((b, 2, 5, 64, 64), generator=g) * 3,
                        "index": ([f"plate/A/1/{pos}/0"] * b, torch.arange(b), torch.full((b,), 2))})
    preds = []
    hook = module.model.register_forward_hook(lambda mod, args, output: preds.append(output.detach().float().cpu()))
    trainer = Trainer()
    out = trainer.test(module, _ListData(batches))
    hook.remove()
    keys = {f"test_metrics/{k}" for k in ("MAE", "MSE", "cosine", "pearson", "r2", "SSIM")}
    assert isinstance(out, list) and len(out) == 1 and set(out[0]) == keys
    assert [v.item() for v in module.logged["position"]] == [7.0, 8.0] and len(module.logged["test_metrics/SSIM"]) == 2
    assert len(preds) == 2 and preds[0].shape == (2, 2, 5, 64, 64)
    # the float64 statements on the module's own predictions, weighted by batch size
    want = dict.fromkeys(keys, 0.0)
    tol = dict.fromkeys(keys, 0.0)
    taps = M.window_taps(21)
    for batch, pred in zip(batches, preds):
        p = pred[:, 0, 2:3].contiguous()
        t = batch["target"][:, 0, 2:3].contiguous()
        w = p.shape[0] / 3.0
        m, bound = _numpy_metrics(p, t)
        for k, v in m.items():
            want[f"test_metrics/{k}"] += w * v
            tol[f"test_metrics/{k}"] += w * bound[k]
        full, yard = _ssim_want(p, t, taps, None, (p.shape[0], 1))
        want["test_metrics/SSIM"] += w * full.mean((1, 2, 3)).mean().item()
        tol["test_metrics/SSIM"] += w * 2 * yard
    for k in keys:
        assert abs(out[0][k] - want[k]) <= tol[k] + 8 * R.U64 * abs(want[k]), (k, out[0][k], want[k], tol[k])
    again = Trainer().test(module, _ListData(batches))
    assert again == out  # bit-identical: fixed-order sums in the bf16 forward and in the metric kernels


def test_print_margins():
    """the worst error / bound ratio of every counted check of this run (the figures of profiles/test_metrics_margins.txt)"""
    for what in sorted(R.MARGINS):
        print(f"worst {what}: {R.MARGINS[what]:.3g}")
