"""GPU: FNet3D on the conv3d / bn3d kernel family (csrc/conv3d.hip) — every op against its torch statement (tests/ref_ops_fnet3d.py),
the fp32 engine against the reference fixture and the statement, the bf16 engine against the autocast yardstick, determinism,
hipGraph capture, the VSUNet surface (fit, padded predict, sliding windows) and a libvsx-only launch check."""

import os
import tempfile

import numpy as np
import pytest
import torch

from tests import ref_fnet3d
from tests import ref_ops_fnet3d as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fnet3d.pt")
TOL = {torch.float32: 2e-4, torch.bfloat16: 2.5e-2}


def _record(tag, *kv):
    """measured yardstick ratios, appended as JSON lines to $VSX_RECORD (when set)"""
    import json

    path = os.environ.get("VSX_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": tag, **dict(zip(kv[::2], kv[1::2]))}) + "\n")


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _rnd(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dt).cuda()


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLD, weights_only=True)


# ------------------------------------------------------------------------------------------------ ops
CONV_CASES = [  # (B, D, H, W, cin, cout, stride / "T")
    (1, 8, 8, 16, 1, 32, 1), (3, 2, 4, 8, 32, 2, 1), (1, 1, 4, 4, 64, 48, 1), (3, 8, 8, 8, 48, 64, 1), (1, 2, 8, 8, 128, 128, 1),
    (3, 8, 8, 16, 32, 64, 2), (1, 2, 4, 4, 64, 128, 2), (1, 8, 8, 8, 2, 32, 2),
    (3, 1, 2, 4, 64, 32, "T"), (1, 4, 4, 8, 128, 64, "T"), (1, 2, 2, 2, 48, 2, "T"),
]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[str(c) for c in CONV_CASES])
def test_conv_ops_match_torch(case, dt):
    """forward (+ bias, stats), the data gradient of the same shape and the weight gradient against the torch statements;
    operands through strided / offset slices"""
    from viscy_amd import ops

    B, D, H, W, cin, cout, st = case
    tr = st == "T"
    stride = 2 if tr else st
    M = B * D * H * W
    Do, Ho, Wo = ((2 * D, 2 * H, 2 * W) if tr else (D // stride, H // stride, W // stride))
    Mo = B * Do * Ho * Wo
    a = _rnd((M, cin + 3), dt, 1)  # operand in columns [3, 3 + cin)
    w = (_rnd((cin, cout, 3, 3, 3) if tr else (cout, cin, 3, 3, 3), torch.float32, 2) * 0.1).contiguous()
    bias = _rnd((cout,), torch.float32, 3)
    out = torch.zeros((Mo, cout + 2), dtype=dt, device="cuda")
    role = "convT" if tr else "conv"
    stats = ops.c3_conv(a, 3, cin, ops.c3_prep(w, role, dt), bias, out, 2, cout, (B, D, H, W), stride, tr, False, True)
    ref = torch.zeros((Mo, cout + 2))
    wq = w.to(dt).float().cpu()
    R.c3_conv(a.float().cpu(), 3, cin, R.c3_prep(wq, role, dt), bias.cpu(), ref, 2, cout, (B, D, H, W), stride, tr)
    assert _rel(out[:, 2:], ref[:, 2:]) <= TOL[dt]
    assert torch.count_nonzero(out[:, :2]) == 0
    z = out[:, 2:].float().cpu().double()
    s = stats.sum(0).cpu().double()
    assert _rel(s[0], z.sum(0)) <= 1e-4 and _rel(s[1], (z * z).sum(0)) <= 1e-4
    # data gradient: the adjoint of the forward, accumulated into an offset slice
    dy = _rnd((Mo, cout), dt, 4)
    if tr:
        role_d, st_d, tr_d = "convT_dgrad", 2, False
    elif stride == 1:
        role_d, st_d, tr_d = "conv_dgrad_s1", 1, False
    else:
        role_d, st_d, tr_d = "conv_dgrad_s2", 2, True
    dx = _rnd((M, cin + 1), dt, 5)
    dx_ref = dx.float().cpu().clone()
    ops.c3_conv(dy, 0, cout, ops.c3_prep(w, role_d, dt), None, dx, 1, cin, (B, Do, Ho, Wo), st_d, tr_d, True)
    R.c3_conv(dy.float().cpu(), 0, cout, R.c3_prep(wq, role_d, dt), None, dx_ref, 1, cin, (B, Do, Ho, Wo), st_d, tr_d, True)
    assert _rel(dx[:, 1:], dx_ref[:, 1:]) <= TOL[dt]
    assert torch.equal(dx[:, 0].float().cpu(), dx_ref[:, 0])
    # weight gradient
    dW = torch.zeros_like(w)
    dW_ref = torch.zeros_like(w).cpu()
    if tr:
        ops.c3_wgrad(a, 3, cin, dy, 0, cout, dW, (B, D, H, W), 2)
        R.c3_wgrad(a.float().cpu(), 3, cin, dy.float().cpu(), 0, cout, dW_ref, (B, D, H, W), 2)
    else:
        ops.c3_wgrad(dy, 0, cout, a, 3, cin, dW, (B, Do, Ho, Wo), stride)
        R.c3_wgrad(dy.float().cpu(), 0, cout, a.float().cpu(), 3, cin, dW_ref, (B, Do, Ho, Wo), stride)
    assert _rel(dW, dW_ref) <= TOL[dt]
    db = torch.zeros(cout, device="cuda")
    ops.c3_colsum(dy, 0, cout, db)
    assert _rel(db, dy.float().cpu().sum(0)) <= (1e-5 if dt == torch.float32 else 1e-3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,C", [(1 * 1 * 2 * 2, 128), (3 * 8 * 8 * 8, 32), (1 * 2 * 4 * 4, 48), (3 * 4 * 4 * 4, 2)])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_batchnorm_ops_match_torch(M, C, dt, training):
    """finalize (batch statistics, running-stat update) + apply / ReLU into an offset slice + backward, against F.batch_norm"""
    from viscy_amd import ops

    z = (_rnd((M, C), dt, 11) * 2 + 0.5).to(dt)
    gamma, beta = _rnd((C,), torch.float32, 12) * 0.1 + 1, _rnd((C,), torch.float32, 13) * 0.1
    rm, rv = _rnd((C,), torch.float32, 14) * 0.1, _rnd((C,), torch.float32, 15).abs() + 0.5
    nbt = torch.zeros((), dtype=torch.long, device="cuda")
    rm_r, rv_r = rm.cpu().clone(), rv.cpu().clone()
    stats = torch.stack([z.float().sum(0), (z.float() ** 2).sum(0)])[None]  # the conv epilogue's partials
    ss = ops.bn3d_finalize(stats, M, C, gamma, beta, rm, rv, nbt, training)
    y = torch.zeros((M, C + 1), dtype=dt, device="cuda")
    ops.bn3d_apply_relu(z, ss, y, 1)
    zr = z.float().cpu().requires_grad_(True)
    yr = torch.relu(torch.nn.functional.batch_norm(zr, rm_r, rv_r, gamma.cpu(), beta.cpu(), training, 0.1, 1e-5))
    assert _rel(y[:, 1:], yr.detach()) <= TOL[dt]
    if training:
        assert _rel(rm, rm_r) <= 1e-5 and _rel(rv, rv_r) <= 1e-5 and int(nbt) == 1
    dy = _rnd((M, C + 2), dt, 16)
    dg, dbt = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dz = ops.bn3d_bwd(dy, 2, z, ss, gamma, dg, dbt, training)
    gam = gamma.cpu().requires_grad_(True)
    bet = beta.cpu().requires_grad_(True)
    zr = z.float().cpu().requires_grad_(True)
    if training:
        yr = torch.relu(torch.nn.functional.batch_norm(zr, None, None, gam, bet, True, 0.1, 1e-5))
    else:
        yr = torch.relu(torch.nn.functional.batch_norm(zr, rm_r, rv_r, gam, bet, False, 0.1, 1e-5))
    yr.backward(dy[:, 2:].float().cpu())
    assert _rel(dz, zr.grad) <= TOL[dt] * 4
    assert _rel(dg, gam.grad) <= TOL[dt] and _rel(dbt, bet.grad) <= TOL[dt]


# ------------------------------------------------------------------------------------------------ engine
def _gpu_model(case, dt, grad_mode="autograd"):
    from viscy_amd.unet3d import Unet3d

    m = Unet3d(**case["kwargs"])
    m.load_state_dict(case["state_dict"], strict=True)
    m = m.cuda().train()
    m.compute_dtype, m.grad_mode = dt, grad_mode
    return m


@pytest.mark.parametrize("name", ["d2_m4_out1", "d3_m2_out2"])
def test_fp32_engine_matches_fixture(golden, name):
    case = golden["cases"][name]
    m = _gpu_model(case, torch.float32)
    y = m(case["x"].cuda())
    assert _rel(y.detach(), case["out"]) <= 1e-3
    (y * case["gout"].cuda()).sum().backward()
    gw = {k: p.grad for k, p in m.named_parameters()}
    # all gradients together at 1e-3; per tensor at 3e-2: the fixture's nets are 2 - 16 channels wide with BatchNorms over 96 - 3072
    # voxels, where a ReLU that flips on fp32 round-off moves a small tensor's gradient by a few 1e-3
    assert _rel(torch.cat([gw[k].flatten() for k in case["grads"]]), torch.cat([g.flatten() for g in case["grads"].values()])) <= 1e-3
    for k, gr in case["grads"].items():
        if k.endswith("proj.bias"):  # feeds a BatchNorm: zero in exact arithmetic
            assert gw[k].abs().max().item() <= 1e-3 * case["grads"][k[:-4] + "weight"].abs().max().item(), k
        else:
            assert _rel(gw[k], gr) <= 3e-2, k
    sd = m.state_dict()
    for k, v in case["buffers_after"].items():
        if v.dtype.is_floating_point:
            assert _rel(sd[k], v) <= 1e-3, k
        else:
            assert int(sd[k]) == int(v), k
    m.eval()
    with torch.no_grad():
        assert _rel(m(case["x"].cuda()), case["out_eval"]) <= 1e-3


def test_autograd_mode_equals_flat_mode_fp32(golden):
    """the same net and input in ``grad_mode = "flat"`` and ``"autograd"``: equal up to the run-to-run floor of the atomic
    reductions, measured here on two identical flat-mode runs, and every parameter receives a ``.grad``"""
    case = golden["cases"]["d3_m2_out2"]
    m = _gpu_model(case, torch.float32, "flat")
    eng = m.engine()
    x, gout = case["x"].cuda(), case["gout"].cuda()

    def flat_run():
        m.grad_mode = "flat"
        eng.flat_grad.zero_()
        m(x).backward(gout)
        return eng.flat_grad.clone()

    g1, g1b = flat_run(), flat_run()
    m.grad_mode = "autograd"
    for p in m.parameters():
        p.grad = None
    kept = eng.flat_grad.clone()
    m(x).backward(gout)
    assert all(p.grad is not None for p in m.parameters())
    assert torch.equal(eng.flat_grad, kept)  # autograd mode leaves the flat buffer alone
    ga = torch.zeros_like(g1)
    for p, o in zip(eng.order, eng.offsets):
        ga[o : o + p.numel()] = p.grad.flatten()
    floor = torch.nn.functional.cosine_similarity(g1, g1b, dim=0).item()
    cos = torch.nn.functional.cosine_similarity(g1, ga, dim=0).item()
    print(f"flat vs flat {floor:.7f}, flat vs autograd {cos:.7f}")
    assert cos > floor - 2e-3, (floor, cos)


def test_fp32_engine_matches_statement_wider():
    """a wider net (vector paths, 64-column tiles, B = 1, deepest level Z = 1) against the statement in fp32"""
    from viscy_amd.unet3d import Unet3d

    torch.manual_seed(3)
    ref = ref_fnet3d.FNet3D(1, 2, depth=3, mult_chan=16).train()
    m = Unet3d(1, 2, depth=3, mult_chan=16)
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.cuda().train()
    m.compute_dtype = torch.float32
    x = torch.randn(1, 1, 8, 16, 32)
    gout = torch.randn(1, 2, 8, 16, 32)
    y = m(x.cuda())
    yr = ref(x)
    assert _rel(y.detach(), yr.detach()) <= 1e-3
    (y * gout.cuda()).sum().backward()
    (yr * gout).sum().backward()
    refp = dict(ref.named_parameters())
    for k, p in m.named_parameters():
        if k.endswith("proj.bias"):
            assert p.grad.abs().max().item() <= 1e-3 * refp[k[:-4] + "weight"].grad.abs().max().item(), k
        else:
            assert _rel(p.grad, refp[k].grad) <= 1e-3, k


def test_bf16_engine_within_autocast_yardstick():
    """bf16 engine error against the fp32 statement <= 1.25 x the error of the statement under torch autocast(bf16), on the
    forward and on the gradients of every weight (fixed seeds)"""
    from viscy_amd.unet3d import Unet3d

    for seed in (0, 1):
        torch.manual_seed(seed)
        ref = ref_fnet3d.FNet3D(1, 1, depth=3, mult_chan=16).cuda().train()
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        g = torch.Generator().manual_seed(10 + seed)
        x = torch.randn((2, 1, 16, 32, 32), generator=g).cuda()
        gout = torch.randn((2, 1, 16, 32, 32), generator=g).cuda()
        y32 = ref(x)
        (y32 * gout).sum().backward()
        g32 = {k: p.grad.clone() for k, p in ref.named_parameters()}
        ref.load_state_dict(sd)
        ref.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            yac = ref(x)
        (yac.float() * gout).sum().backward()
        gac = {k: p.grad.clone() for k, p in ref.named_parameters()}
        m = Unet3d(1, 1, depth=3, mult_chan=16)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train()
        m.compute_dtype = torch.bfloat16
        yb = m(x)
        (yb * gout).sum().backward()
        out_ratio = _rel(yb.detach(), y32.detach()) / _rel(yac.detach(), y32.detach())
        ks = [k for k, _ in m.named_parameters() if k.endswith(".weight") and "norm" not in k]
        gb = dict(m.named_parameters())
        flat = lambda d: torch.cat([(d[k].grad if hasattr(d[k], "grad") and d[k].grad is not None else d[k]).flatten().float().cpu()
                                    for k in ks])
        grad_ratio = _rel(flat(gb), flat(g32)) / _rel(flat(gac), flat(g32))
        ratios = {k: _rel(gb[k].grad, g32[k]) / max(_rel(gac[k], g32[k]), 1e-6) for k in ks}
        w = max(ratios.values())
        _record("fnet3d_bf16_yardstick", "seed", seed, "out_ratio", out_ratio, "grad_ratio", grad_ratio, "worst_layer_ratio", w)
        assert out_ratio <= 1.25 and grad_ratio <= 1.25, (out_ratio, grad_ratio)
        # per layer: the bottleneck of this net averages over 2 x 4 x 4 voxels, where both errors are a handful of roundings
        assert w <= 1.5, sorted(ratios.items(), key=lambda kv: -kv[1])[:4]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_is_bit_identical(dt):
    from viscy_amd.unet3d import Unet3d

    torch.manual_seed(0)
    m = Unet3d(1, 1, depth=4, mult_chan=8).cuda()
    m.compute_dtype = dt
    x = torch.randn((3, 1, 16, 32, 48), device="cuda")
    for mode in ("train", "eval"):
        getattr(m, mode)()
        with torch.no_grad():
            a, b = m(x), m(x)
        assert torch.equal(a, b), mode


def test_graph_step_matches_eager():
    """TrainStep(use_graph=True) against eager over 3 steps: losses, parameters and running statistics"""
    from viscy_amd.losses import MixedLoss
    from viscy_amd.optim import FlatAdamW
    from viscy_amd.step import TrainStep
    from viscy_amd.unet3d import Unet3d

    g = torch.Generator().manual_seed(1)
    xs = [torch.randn((2, 1, 8, 16, 16), generator=g).cuda() for _ in range(3)]
    ts = [torch.rand((2, 1, 8, 16, 16), generator=g).cuda() for _ in range(3)]
    res = {}
    for use_graph in (False, True):
        torch.manual_seed(0)
        m = Unet3d(1, 1, depth=3, mult_chan=8).cuda().train()
        m.compute_dtype, m.grad_mode = torch.float32, "flat"
        step = TrainStep(m, MixedLoss(0.0, 1.0, 0.0), FlatAdamW(m.engine(), lr=1e-3), use_graph=use_graph)
        losses = [float(step(x, t)) for x, t in zip(xs, ts)]
        torch.cuda.synchronize()
        res[use_graph] = (losses, m.engine().flat.clone(), {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_b" in k})
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=1e-5)
    assert _rel(res[True][1], res[False][1]) <= 1e-5
    for k, v in res[False][2].items():
        assert torch.allclose(res[True][2][k].double(), v.double(), rtol=1e-5, atol=1e-7), k
    assert all(int(v) == 3 for k, v in res[True][2].items() if "num_b" in k)


# ------------------------------------------------------------------------------------------------ VSUNet
def _vsunet(depth=2, mult=8, out=1, z=16):
    from viscy_amd.vsunet import VSUNet

    return VSUNet("FNet3D", dict(in_channels=1, out_channels=out, depth=depth, mult_chan=mult, in_stack_depth=z), lr=1e-3)


def test_trainer_fit_over_hcs_plate():
    from viscy_amd.data import HCSDataModule, write_hcs_plate
    from viscy_amd.trainer import Trainer
    from viscy_amd.transforms import NormalizeSampled

    d = tempfile.mkdtemp()
    rng = np.random.default_rng(3)
    pos = {f"A/{c}/0": rng.random((1, 2, 16, 32, 48), dtype=np.float32) for c in (1, 2, 3)}
    meta = {ch: {"fov_statistics": {"mean": 0.5, "std": 0.29}} for ch in ("Phase3D", "Nuclei")}
    write_hcs_plate(os.path.join(d, "t.zarr"), pos, ["Phase3D", "Nuclei"], norm_meta=meta)
    dm = HCSDataModule(os.path.join(d, "t.zarr"), "Phase3D", "Nuclei", z_window_size=16, batch_size=2, num_workers=0,
                       yx_patch_size=(32, 48), split_ratio=0.67, normalizations=[NormalizeSampled(["Phase3D"], "fov_statistics")])
    torch.manual_seed(0)
    model = _vsunet()
    before = {k: v.clone() for k, v in model.model.state_dict().items()}
    tr = Trainer(max_epochs=2, precision="32-true", seed=3)
    tr.fit(model, dm)
    assert tr.finished and all(torch.isfinite(v) for v in model.logged["loss/train"])
    after = model.model.state_dict()
    assert not torch.equal(after["inconv.weight"].cpu(), before["inconv.weight"])
    assert not torch.equal(after["_encoder_blocks.0.0.block1.norm.running_mean"].cpu(),
                           before["_encoder_blocks.0.0.block1.norm.running_mean"])
    assert int(after["_encoder_blocks.0.0.block1.norm.num_batches_tracked"]) >= 2


def test_predict_pads_z_y_x_and_crops_back():
    from viscy_amd.vsunet import _center_crop_to_shape

    torch.manual_seed(0)
    vs = _vsunet(depth=2, mult=8, out=2, z=10).cuda()
    vs.model.eval()
    x = torch.randn((1, 1, 10, 30, 45)).cuda()
    with torch.no_grad():
        p = vs.predict_step({"source": x}, 0)
        assert p.shape == (1, 2, 10, 30, 45)
        xp = torch.nn.functional.pad(x, (1, 2, 1, 1, 1, 1))  # 10 -> 12, 30 -> 32, 45 -> 48: divisible by 4
        full = vs.model(xp)
        assert torch.equal(p, _center_crop_to_shape(full, (10, 30, 45)))
        vs.predict_graph = True
        pg = vs.predict_step({"source": x}, 0)
        assert _rel(pg, p) <= 1e-6
        vs.predict_graph = False
        vs.test_time_augmentations = True
        pt = vs.predict_step({"source": x}, 0)
        assert pt.shape == p.shape and torch.isfinite(pt).all()


def test_predict_sliding_windows():
    torch.manual_seed(0)
    vs = _vsunet(depth=2, mult=8, out=1, z=8).cuda()
    vs.model.eval()
    x = torch.randn((1, 1, 12, 32, 32)).cuda()
    with torch.no_grad():
        out = vs.predict_sliding_windows(x, out_channel=1, step=2)
        first = vs.predict_step({"source": x[:, :, :8].contiguous()}, 0)
    assert out.shape == (1, 1, 12, 32, 32) and torch.isfinite(out).all()
    assert torch.equal(out[:, :, :2], first[:, :, :2])


OURS = ("conv3d_", "bn3d_", "adamw", "fill_f32", "loss_", "ssim_")


def test_fnet3d_training_step_launches_only_libvsx_kernels():
    """one eager bf16 training step (forward, MSE, backward, AdamW) under torch.profiler launches only libvsx kernels, except the
    autograd loss seed"""
    from torch.profiler import ProfilerActivity, profile

    from viscy_amd.losses import MixedLoss
    from viscy_amd.optim import FlatAdamW
    from viscy_amd.step import TrainStep
    from viscy_amd.unet3d import Unet3d

    torch.manual_seed(0)
    m = Unet3d(1, 1, depth=3, mult_chan=8).cuda().train()
    m.compute_dtype, m.grad_mode = torch.bfloat16, "flat"
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 1, 8, 32, 32), generator=g).cuda()
    t = torch.rand((2, 1, 8, 32, 32), generator=g).cuda()
    step = TrainStep(m, MixedLoss(0.0, 1.0, 0.0), FlatAdamW(m.engine(), lr=1e-4), use_graph=False, static_inputs=True)
    for _ in range(2):
        step(x, t)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(x, t)
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")]
    assert any("conv3d_igemm" in n for n in names) and any("bn3d_" in n for n in names)
    foreign = [n[:90] for n in names if not any(o in n for o in OURS)]
    assert len(foreign) <= 1 and all("FillFunctor" in n for n in foreign), foreign
