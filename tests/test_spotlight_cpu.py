"""CPU: the float64 restatement of SpotlightLoss (tests/ref_spotlight.py) against what the reference computed
(tests/golden/spotlight.pt, written by tools/gen_golden_spotlight.py), and the parts of viscy_amd.SpotlightLoss that need no GPU."""

import os

import numpy as np
import pytest
import torch

from tests import ref_spotlight as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "spotlight.pt"), weights_only=True)


def test_golden_covers_the_case_table(golden):
    assert set(golden["cases"]) == set(RS.CASES) and set(golden["otsu"]) == set(RS.OTSU_CASES)
    for name, case in RS.CASES.items():
        assert tuple(golden["cases"][name]["shape"]) == case["shape"], name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "spotlight.pt")) < 256 * 1024


def test_restatement_reproduces_every_golden_loss_and_gradient(golden):
    """Per case the reference's own fp32-vs-float64 deviation is asserted <= 1e-5 relative, and the restatement is within that
    deviation of the reference's fp32 result.  Against the reference run on float64 inputs the restatement agrees to 2^-23
    relative, not to float64 round-off: the reference's mask is ``.float()`` whatever the inputs are, so it rounds F + eps to
    fp32 (relative error <= 2^-24 + eps / F, below 2^-23 for the F >= 17 of every row of the table that has foreground).
    Worst deviations of the reference over the table (torch 2.10, CPU): loss 2.2e-7 (tiny4d_thr), gradient 6.5e-7 of the largest
    entry (chunk5_bool)."""
    worst_l = worst_g = 0.0
    for name in RS.CASES:
        inp, g = RS.build(name), golden["cases"][name]
        loss, grad = RS.loss_and_grad(inp["pred"], inp["target"], inp["fg_mask"], inp["fg_threshold"], gout=inp["gout"])
        gs = grad.reshape(-1)[RS.grad_sample_index(grad.numel())]
        l32, l64 = g["loss32"].double().item(), g["loss64"].item()
        g32, g64 = g["grad32"].double(), g["grad64"]
        dev_l = abs(l32 - l64) / abs(l64)
        gmax = g64.abs().max().item()
        dev_g = (g32 - g64).abs().max().item() / gmax
        print(f"{name:18s} reference fp32 vs float64: loss {dev_l:.2e}  gradient {dev_g:.2e} of max |grad|")
        worst_l, worst_g = max(worst_l, dev_l), max(worst_g, dev_g)
        assert dev_l <= 1e-5 and dev_g <= 1e-5, name
        e64_l, e64_g = abs(loss.item() - l64) / abs(l64), (gs - g64).abs().max().item() / gmax
        print(f"{'':18s} restatement vs reference float64: loss {e64_l:.2e}  gradient {e64_g:.2e}")
        assert e64_l <= 2.0**-23 and e64_g <= 2.0**-23, name
        assert abs(loss.item() - l32) <= (dev_l + 2.0**-23) * abs(l64), name
        assert (gs - g32).abs().max().item() <= (dev_g + 2.0**-23) * gmax, name
        assert torch.isfinite(grad).all(), name
    print(f"worst reference fp32 deviation: loss {worst_l:.2e}, gradient {worst_g:.2e}")


def test_no_real_rows_gives_mse_only_and_clamp_ends_pass_the_gradient():
    inp = RS.build("no_real")
    loss, grad = RS.loss_and_grad(inp["pred"], inp["target"], inp["fg_mask"])
    p, t = inp["pred"].double(), inp["target"].double()
    n = p[0, 0].numel()
    mse = ((p - t) ** 2).reshape(2, -1)
    want = 0.5 * (mse[0].sum() / (n + 1e-6) + mse[1].mean()) / 2
    assert abs(loss.item() - want.item()) <= 1e-14
    # sigmoid_k = -0.95: ds/dp is 39 at p = 0 and 1 / 39 at p = 1, zero just outside [0, 1]
    k = -0.95
    for p0, want in ((0.0, 39.0), (1.0, 0.02564102564), (1.0 + 2.0**-10, 0.0), (-1e-30, 0.0)):
        den = k - 2 * k * abs(p0) + 1
        raw = (p0 - k * p0) / den
        ds = (1 - k * k) / den**2 if 0 <= raw <= 1 else 0.0
        assert abs(ds - want) <= 1e-9, (p0, ds)


def test_golden_thresholds_are_reproduced_exactly(golden):
    """Bit for bit on the integer-grid targets, where every bin centre is exact in fp32.  On the float fixture the restatement
    picks the reference's bin, and its centre lo + (idx + 0.5) (hi - lo) / 256, rounded once from float64, is within 2^-21
    max(|lo|, |hi|) of the reference's, which averages two fp32 ``linspace`` edges (three fp32 roundings of values below
    max(|lo|, |hi|), 2^-24 relative each, with room to spare): it cannot be bit-equal to it."""
    for name in ("grid", "grid_multi"):
        thr = RS.otsu_thresholds(RS.otsu_target(name))
        print(name, thr.flatten().tolist())
        assert torch.equal(thr, golden["otsu"][name]["thr"]), name
    assert golden["otsu"]["grid"]["thr"].flatten().tolist() == [59.5, 59.5, 59.5, 7.0]
    assert golden["otsu"]["grid_multi"]["thr"].flatten().tolist() == [59.5, 59.5]
    t = RS.otsu_target("bimodal")
    thr, want = RS.otsu_thresholds(t).flatten().double(), golden["otsu"]["bimodal"]["thr"].flatten().double()
    rows = t.reshape(thr.numel(), -1).double()
    lo, hi = rows.min(1).values, rows.max(1).values
    width = (hi - lo) / 256
    print("bimodal", thr.tolist(), "reference", want.tolist())
    assert torch.equal(torch.floor((thr - lo) / width), torch.floor((want - lo) / width))  # the same bin
    assert ((thr - want).abs() <= 2.0**-21 * torch.maximum(lo.abs(), hi.abs())).all()


def test_binning_form_b_gives_histc_counts():
    t = RS.otsu_target("bimodal")
    for row in t.reshape(t.shape[0] * t.shape[1], -1):
        lo, hi = row.min(), row.max()
        want = torch.histc(row, bins=256, min=lo.item(), max=hi.item()).long()
        got = np.bincount(RS.bin_index(row.numpy(), np.float32(lo.item()), np.float32(hi.item()), 256), minlength=256)
        assert want.sum().item() == row.numel()
        assert np.array_equal(got, want.numpy())


def test_constructor_defaults_errors_and_export():
    import inspect

    import viscy_amd
    from viscy_amd.losses import SpotlightLoss

    assert viscy_amd.SpotlightLoss is SpotlightLoss and "SpotlightLoss" in viscy_amd.__all__
    sig = inspect.signature(SpotlightLoss.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("lambda_mse", 0.5), ("sigmoid_k", -0.95), ("eps", 1e-6), ("fg_threshold", None)]
    assert list(inspect.signature(SpotlightLoss.forward).parameters) == ["self", "pred", "target", "fg_mask"]
    fn = SpotlightLoss()
    assert (fn.lambda_mse, fn.sigmoid_k, fn.eps, fn.fg_threshold) == (0.5, -0.95, 1e-6, None)
    for kw, msg in ((dict(sigmoid_k=0.0), "sigmoid_k must be in"), (dict(sigmoid_k=-1.0), "sigmoid_k must be in"),
                    (dict(lambda_mse=0.0), "lambda_mse must be in"), (dict(lambda_mse=1.0), "lambda_mse must be in"),
                    (dict(eps=0.0), "eps must be > 0")):
        with pytest.raises(ValueError, match=msg):
            SpotlightLoss(**kw)


def test_no_cpu_fallback_and_shape_validation():
    from viscy_amd.losses import SpotlightLoss

    fn = SpotlightLoss(fg_threshold=0.0)
    x = torch.zeros(1, 2, 3, 8, 8)
    with pytest.raises(RuntimeError, match=r"SpotlightLoss runs on MI355X HIP kernels only \(no CPU / eager fallback\)"):
        fn(x, x)
    with pytest.raises(RuntimeError, match="no CPU"):
        fn(x[:, :, 0], x[:, :, 0], fg_mask=x[:, :, 0] > 0)
    with pytest.raises(ValueError, match="same shape"):
        fn(x, x[:, :1])
    with pytest.raises(ValueError, match="dimensions"):
        fn(x[0, 0], x[0, 0])
    with pytest.raises(ValueError, match="dimensions"):
        fn(x[None], x[None])
    with pytest.raises(ValueError, match="empty"):
        fn(x[:0], x[:0])
    with pytest.raises(ValueError, match="fg_mask"):
        fn(x, x, fg_mask=x[:, :1] > 0)


def test_yaml_seam_builds_a_vsunet_with_the_spotlight_loss():
    import yaml

    from viscy_amd import config
    from viscy_amd.losses import SpotlightLoss
    from viscy_amd.vsunet import VSUNet

    cfg = yaml.safe_load("""
model:
  class_path: cytoland.engine.VSUNet
  init_args:
    architecture: UNeXt2
    model_config:
      in_channels: 1
      out_channels: 2
      in_stack_depth: 5
      backbone: convnextv2_atto
    loss_function:
      class_path: viscy_utils.losses.SpotlightLoss
      init_args:
        lambda_mse: 0.5
        sigmoid_k: -0.95
        fg_threshold: 0.0
""")
    module = config.instantiate(cfg["model"])
    assert isinstance(module, VSUNet) and type(module.loss_function) is SpotlightLoss
    assert module._loss_accepts_fg_mask is True
    fn = module.loss_function
    assert (fn.lambda_mse, fn.sigmoid_k, fn.eps, fn.fg_threshold) == (0.5, -0.95, 1e-6, 0.0)
    other = config.instantiate({"class_path": "viscy_utils.losses.spotlight.SpotlightLoss"})
    assert type(other) is SpotlightLoss and other.fg_threshold is None
