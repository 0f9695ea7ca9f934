"""GPU: viscy_amd.SpotlightLoss (csrc/spotlight.hip) against the float64 restatement of tests/ref_spotlight.py on the same inputs.

Bounds: loss 2e-6 relative (that of test_masked_mse_loss_vs_oracle); fp32 gradient rtol 1e-5, atol 1e-9 + 1e-6 max|grad|; with a
bf16 prediction (inputs rounded to bf16 first) the same loss bound and the gradient within one bf16 rounding, rtol 2^-8.  Where the
reference's own fp32 result (tests/golden/spotlight.pt) is further from its float64 result than a bound, the case gets four times
the reference's deviation; both are printed."""

import functools
import os

import pytest
import torch

from tests import ref_spotlight as RS

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "spotlight.pt"), weights_only=True)


@functools.lru_cache(maxsize=None)
def _want(name):
    """the restatement's (loss, gradient) of a case, computed once"""
    inp = RS.build(name)
    return RS.loss_and_grad(inp["pred"], inp["target"], inp["fg_mask"], inp["fg_threshold"], gout=inp["gout"])


def _bounds(name):
    """(relative loss bound, factor on the gradient tolerance) from the reference's own fp32-vs-float64 deviation"""
    g = _golden()["cases"][name]
    l32, l64 = g["loss32"].double().item(), g["loss64"].item()
    g32, g64 = g["grad32"].double(), g["grad64"]
    dev_l = abs(l32 - l64) / abs(l64)
    tol = 1e-5 * g64.abs() + 1e-9 + 1e-6 * g64.abs().max()
    ratio = ((g32 - g64).abs() / tol).max().item()
    loss_bound = 2e-6 if dev_l <= 2e-6 else 4 * dev_l
    grad_factor = 1.0 if ratio <= 1.0 else 4 * ratio
    print(f"{name}: reference fp32 vs float64: loss {dev_l:.2e} (bound {loss_bound:.2e}), gradient {ratio:.2f} of the tolerance "
          f"(factor {grad_factor:.2f})")
    return loss_bound, grad_factor


def _run(name):
    from viscy_amd.losses import SpotlightLoss

    inp, case = RS.build(name), RS.CASES[name]
    pred = inp["pred"].to(DEV)
    if case.get("bf16"):
        pred = pred.bfloat16()
    pred.requires_grad_(True)
    mask = inp["fg_mask"].to(DEV) if inp["fg_mask"] is not None else None
    loss = SpotlightLoss(fg_threshold=inp["fg_threshold"])(pred, inp["target"].to(DEV), fg_mask=mask)
    (loss * inp["gout"]).backward()
    assert loss.dtype == torch.float32 and loss.ndim == 0 and pred.grad.dtype == pred.dtype
    return loss.item(), pred.grad.detach().cpu()


def _check(name):
    want_l, want_g = _want(name)
    loss_bound, grad_factor = _bounds(name)
    got_l, got_g = _run(name)
    err_l = abs(got_l - want_l.item()) / abs(want_l.item())
    gmax = want_g.abs().max()
    atol = 1e-9 + 1e-6 * gmax
    rtol = 2.0**-8 if RS.CASES[name].get("bf16") else 1e-5
    err_g = ((got_g.double() - want_g).abs() / (rtol * want_g.abs() + atol)).max().item()
    print(f"{name}: loss {got_l:.7f}  relative error {err_l:.2e} (bound {loss_bound:.1e});  gradient error {err_g:.3f} of the "
          f"tolerance (rtol {rtol:.1e}, atol {atol:.1e})")
    assert torch.isfinite(got_g).all()
    assert err_l <= loss_bound
    assert err_g <= grad_factor
    return got_l, got_g


@pytest.mark.parametrize("name", list(RS.CASES))
def test_loss_and_gradient_vs_float64(name):
    """every row of the case table: the base shape in all mask modes (mask as bool, uint8, float32), 4-D N = 63, odd N (row
    starts off the vector grid), N = 2 CHUNK + 5 and N = 83 200 (several workgroups per row, ragged last one), mixed rows with
    gout = 3, no real row, the clamp ends, Otsu mode on integer-grid targets with a constant row; fp32 and bf16 predictions"""
    _check(name)


def test_chunk_constant_is_the_one_the_table_was_built_for():
    from viscy_amd import ops

    n = RS.CASES["chunk5_bool"]["shape"][-1]
    assert ops.SPOTLIGHT_CHUNK == RS.SPOTLIGHT_CHUNK and n == 2 * ops.SPOTLIGHT_CHUNK + 5
    rows = 2
    words = ops.spotlight_workspace_floats(rows, n)
    assert words == 2 * (rows * 3 * 5 + rows * 6)  # three workgroups per row, five float64 partials each, six per row


def test_mixed_rows_and_no_real_rows_coefficients():
    """rows without foreground take the unmasked MSE, rows that are not "real" (all ones, all zeros) get no Dice gradient; with
    no real row at all the Dice term is exactly 0, decided on the device: the loss is the MSE part and nothing is NaN"""
    from viscy_amd import ops

    inp = RS.build("mixed_rows")
    loss, coef = ops.spotlight_fwd(inp["pred"].to(DEV), inp["target"].to(DEV), inp["fg_mask"].to(DEV))
    coef = coef.cpu()
    n = inp["pred"][0, 0].numel()
    assert (coef[[0, 3], 0] > 0).all() and (coef[[0, 3], 1] == 0).all()                     # real masks: masked MSE and Dice
    assert (coef[[0, 3], 2] < 0).all() and (coef[[0, 3], 3] > 0).all()
    assert coef[1].tolist()[1:] == [0.0, 0.0, 0.0] and coef[1, 0] > 0                       # all ones: masked MSE, no Dice
    assert coef[2].tolist() == [0.0, pytest.approx(2 * 0.5 / 4 / n, rel=1e-6), 0.0, 0.0]    # all zeros: unmasked MSE, no Dice
    inp = RS.build("no_real")
    p, t = inp["pred"].to(DEV), inp["target"].to(DEV)
    loss, coef = ops.spotlight_fwd(p, t, inp["fg_mask"].to(DEV))
    assert torch.isfinite(loss) and torch.isfinite(coef).all() and (coef[:, 2:] == 0).all()
    mse = ((p.double() - t.double()) ** 2).reshape(2, -1)
    want = 0.5 * (mse[0].sum() / (n + 1e-6) + mse[1].mean()) / 2
    assert abs(loss.item() - want.item()) <= 2e-6 * want.item()
    got_l, got_g = _run("no_real")
    want_g = (0.5 / 2 * 2 * (p.double() - t.double()).reshape(2, -1) * torch.tensor([[1 / (n + 1e-6)], [1 / n]], device=DEV)).cpu()
    torch.testing.assert_close(got_g.double().reshape(2, -1), want_g, rtol=1e-5, atol=1e-9)


def test_clamp_ends_pass_the_gradient_inclusively():
    """at p = 0 and p = 1 exactly the Dice gradient is there (s' = 39 and 1 / 39 for k = -0.95), just outside it is not: on top
    of the comparison with float64, the Dice part is isolated by differencing against the MSE-only gradient"""
    for name in ("clamp_ends", "clamp_ends_bf16"):
        inp = RS.build(name)
        _, got_g = _run(name)
        _, want_g = _want(name)
        p = inp["pred"].reshape(-1)
        for v, inside in ((0.0, True), (1.0, True)):
            idx = (p == v).nonzero().flatten()
            assert idx.numel() >= 4
            m = inp["fg_mask"].reshape(-1)[idx]
            assert m.any() and (~m).any()  # both mask values at the ends
        _, mse_only = RS.loss_and_grad(inp["pred"], inp["target"], inp["fg_mask"], lambda_mse=1.0)
        dice_part = (want_g - 0.5 * mse_only).reshape(-1)
        ends = ((p == 0.0) | (p == 1.0))
        outside = (p < 0) | (p > 1)
        assert (dice_part[ends].abs() > 0).all() and (dice_part[outside].abs() <= 1e-12 * want_g.abs().max()).all()
        rtol = 2.0**-8 if "bf16" in name else 1e-5
        g = got_g.double().reshape(-1)
        assert ((g - want_g.reshape(-1)).abs() <= rtol * want_g.reshape(-1).abs() + 1e-9 + 1e-6 * want_g.abs().max())[ends | outside].all()


@pytest.mark.parametrize("name", ["grid", "grid_multi"])
def test_otsu_thresholds_integer_grid_exact(name):
    """every binning formula is exact on the integer grid 0..256: the reference gives 59.5 for every row (7.0 for the constant
    row, lo == hi), and so must the device, bit for bit"""
    from viscy_amd import ops

    t = RS.otsu_target(name)
    thr = ops.otsu_threshold(t.to(DEV)).cpu()
    want = _golden()["otsu"][name]["thr"]
    print(name, thr.flatten().tolist())
    assert thr.shape == want.shape == t.shape[:2] and thr.dtype == torch.float32
    assert torch.equal(thr, want)
    assert set(want.flatten().tolist()) <= {59.5, 7.0}
    assert torch.equal(thr, RS.otsu_thresholds(t))


def test_otsu_thresholds_float_bimodal_within_one_bin():
    from viscy_amd import ops

    t = RS.otsu_target("bimodal")
    thr = ops.otsu_threshold(t.to(DEV)).cpu().flatten().double()
    want = _golden()["otsu"]["bimodal"]["thr"].flatten().double()
    rows = t.reshape(thr.numel(), -1).double()
    width = (rows.max(1).values - rows.min(1).values) / 256
    print("device", thr.tolist(), "reference", want.tolist(), "restatement", RS.otsu_thresholds(t).flatten().tolist())
    assert ((thr - want).abs() <= width).all()
    # a 4-D target and a bin count of its own go through the same kernels
    t4 = t[:, :, 0].contiguous()
    thr4 = ops.otsu_threshold(t4.to(DEV), n_bins=64).cpu()
    assert torch.equal(thr4, RS.otsu_thresholds(t4, 64))


def test_bit_identical_from_run_to_run():
    from viscy_amd.losses import SpotlightLoss

    g = torch.Generator().manual_seed(5)
    shape = (4, 2, 5, 64, 64)
    t = RS.bimodal_target(shape, 6).to(DEV)
    p0 = (t + 0.3 * torch.randn(shape, generator=g).to(DEV))
    mask = (torch.rand(shape, generator=g) < 0.4).to(DEV)
    for fn, m in ((SpotlightLoss(), mask), (SpotlightLoss(), None)):  # mask mode, Otsu mode
        res = []
        for _ in range(2):
            p = p0.clone().requires_grad_(True)
            loss = fn(p, t, fg_mask=m)
            loss.backward()
            res.append((loss.detach().clone(), p.grad.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert torch.isfinite(res[0][0]) and res[0][1].abs().max() > 0


def test_workspace_needs_no_initialisation():
    from viscy_amd import ops

    inp = RS.build("multi_uint8")
    p, t, m = inp["pred"].to(DEV), inp["target"].to(DEV), inp["fg_mask"].to(DEV)
    rows, n = 2, p[0, 0].numel()
    loss0, coef0 = ops.spotlight_fwd(p, t, m)
    ws = torch.full((ops.spotlight_workspace_floats(rows, n) + 7,), float("nan"), dtype=torch.float32, device=DEV)
    loss1, coef1 = ops.spotlight_fwd(p, t, m, workspace=ws)
    assert torch.equal(loss0, loss1) and torch.equal(coef0, coef1) and torch.isfinite(loss1)
    assert torch.isnan(ws[-7:]).all()  # nothing is written past the size the query gives
    with pytest.raises(ValueError, match="workspace"):
        ops.spotlight_fwd(p, t, m, workspace=ws[:16])


KW_SMALLEST = dict(in_channels=1, out_channels=2, in_stack_depth=5, backbone="convnextv2_atto", head_pool=True)


@pytest.mark.parametrize("mode", ["fixed_threshold", "otsu"])
def test_captured_step_matches_eager(mode):
    """three steps of TrainStep(use_graph=True) with the loss inside the capture (no mask: fixed threshold, then Otsu) against
    three eager steps; bound of test_graph_captured_contrastive_and_pretraining_steps_match_eager"""
    from viscy_amd.losses import SpotlightLoss
    from viscy_amd.optim import FlatAdamW
    from viscy_amd.step import TrainStep
    from viscy_amd.unext2 import UNeXt2

    g = torch.Generator().manual_seed(1)
    xs = [torch.randn((2, 1, 5, 64, 96), generator=g).cuda() for _ in range(3)]
    ts = [(torch.randn((2, 2, 5, 64, 96), generator=g) + 3.0 * (torch.rand((2, 2, 5, 64, 96), generator=g) < 0.3)).cuda()
          for _ in range(3)]
    traj = {}
    for use_graph in (False, True):
        torch.manual_seed(0)
        m = UNeXt2(**KW_SMALLEST).cuda().train()
        m.compute_dtype, m.grad_mode = torch.float32, "flat"
        crit = SpotlightLoss(fg_threshold=0.0) if mode == "fixed_threshold" else SpotlightLoss()
        step = TrainStep(m, crit, FlatAdamW(m.engine(), lr=1e-3), use_graph=use_graph)
        traj[use_graph] = [float(step(x, t)) for x, t in zip(xs, ts)]
        torch.cuda.synchronize()
        if use_graph:
            assert step.graphs is not None
    print(mode, traj)
    assert all(x == x for x in traj[True])
    assert all(abs(x - y) <= 2e-3 * abs(x) + 1e-5 for x, y in zip(traj[False], traj[True])), traj


def test_masked_batch_through_vsunet_training_step():
    """a batch that carries fg_mask no longer raises: VSUNet.training_step returns what the op-level call gives on the same
    prediction"""
    from viscy_amd import ops
    from viscy_amd.losses import SpotlightLoss
    from viscy_amd.vsunet import VSUNet

    torch.manual_seed(0)
    vs = VSUNet(architecture="UNeXt2", model_config=dict(KW_SMALLEST), loss_function=SpotlightLoss(fg_threshold=0.0)).cuda().train()
    vs.model.compute_dtype = torch.float32
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 1, 5, 64, 96), generator=g).cuda()
    t = torch.randn((2, 2, 5, 64, 96), generator=g).cuda()
    mask = (torch.rand((2, 2, 5, 64, 96), generator=g) < 0.4).to(torch.uint8).cuda()
    loss = vs.training_step({"source": x, "target": t, "fg_mask": mask}, 0)
    loss.backward()
    assert torch.isfinite(loss) and any(p.grad is not None and p.grad.abs().max() > 0 for p in vs.parameters())
    with torch.no_grad():
        pred = vs(x)
    want, _ = ops.spotlight_fwd(pred.float().contiguous(), t, mask)
    thr_loss, _ = ops.spotlight_fwd(pred.float().contiguous(), t, None, torch.zeros(4, device=DEV))
    print(loss.item(), want.item(), thr_loss.item())
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    assert abs(thr_loss.item() - want.item()) > 1e-3 * abs(want.item())  # the mask, not the threshold, decided the foreground
