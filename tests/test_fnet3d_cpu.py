"""CPU: FNet3D (viscy_amd.unet3d) — state-dict surface and initialisation against the reference fixture, the torch statement
(tests/ref_fnet3d.py) against the fixture, the kernel schedule (viscy_amd.engine_unet3d with the torch ops of
tests/ref_ops_fnet3d.py) against autograd of the statement, guards and the recipe YAML."""

import math
import os

import pytest
import torch

from tests import ref_fnet3d, ref_ops_fnet3d

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fnet3d.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLD, weights_only=True)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("depth", [3, 4])
def test_state_dict_keys_shapes_and_count(golden, depth):
    from viscy_amd.unet3d import Unet3d

    net = Unet3d(in_channels=1, out_channels=1, depth=depth, mult_chan=32, in_stack_depth=32)
    sd = net.state_dict()
    full = golden["full"][depth]
    assert list(sd.keys()) == full["keys"]
    assert [list(v.shape) for v in sd.values()] == full["shapes"]
    n = sum(p.numel() for p in net.parameters())
    assert n == full["numel"] == {3: 8771073, 4: 35318529}[depth]
    assert len(sd) == {3: 114, 4: 146}[depth]
    assert net.num_blocks == depth and net.downsamples_z is True
    assert net.in_stack_depth == 32 and net.out_stack_depth == 32


def test_load_state_dict_both_ways(golden):
    from viscy_amd.unet3d import Unet3d

    for case in golden["cases"].values():
        kw = case["kwargs"]
        net = Unet3d(**kw)
        net.load_state_dict(case["state_dict"], strict=True)
        ref = ref_fnet3d.FNet3D(**kw)
        ref.load_state_dict(net.state_dict(), strict=True)
        for k, v in ref.state_dict().items():
            assert torch.equal(v, case["state_dict"][k]), k


def test_initialisation_distributions():
    from viscy_amd.unet3d import Unet3d

    torch.manual_seed(0)
    net = Unet3d(depth=3, mult_chan=16)
    convs = [m for m in net.modules() if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d))]
    w = torch.cat([m.weight.detach().flatten() for m in convs])
    assert abs(w.mean().item()) < 1e-3 and abs(w.std().item() - 0.02) < 1e-3
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    g = torch.cat([m.weight.detach() for m in bns])
    assert abs(g.mean().item() - 1.0) < 5e-3 and abs(g.std().item() - 0.02) < 5e-3
    assert all(torch.count_nonzero(m.bias) == 0 for m in bns)
    for m in convs:  # torch default bias: uniform +-1/sqrt(fan_in); ConvTranspose3d takes fan_in from weight dim 1 (= Cout * 27)
        fan_in = m.weight.shape[1] * 27
        bound = 1 / math.sqrt(fan_in)
        b = m.bias.detach()
        assert b.abs().max().item() <= bound
        if b.numel() >= 64:
            assert b.abs().max().item() > 0.8 * bound
    up = net._upsamples[0]
    assert up.weight.shape[1] == 64 and up.bias.abs().max().item() <= 1 / math.sqrt(64 * 27)


@pytest.mark.parametrize("name", ["d2_m4_out1", "d3_m2_out2"])
def test_statement_reproduces_fixture(golden, name):
    case = golden["cases"][name]
    ref = ref_fnet3d.FNet3D(**case["kwargs"]).train()
    ref.load_state_dict(case["state_dict"], strict=True)
    out = ref(case["x"])
    assert _rel(out.detach(), case["out"]) <= 1e-6
    (out * case["gout"]).sum().backward()
    for k, p in ref.named_parameters():
        gr = case["grads"][k]
        tol = 1e-6 * max(gr.abs().max().item(), 1e-3)
        assert (p.grad - gr).abs().max().item() <= max(tol, 1e-6 * case["grads"][k.replace("bias", "weight")].abs().max().item()), k
    sd = ref.state_dict()
    for k, v in case["buffers_after"].items():
        if v.dtype.is_floating_point:
            assert _rel(sd[k], v) <= 1e-6, k
        else:
            assert torch.equal(sd[k], v), k
    ref.eval()
    with torch.no_grad():
        assert _rel(ref(case["x"]), case["out_eval"]) <= 1e-6


def _engine_run(net, x, gout):
    eng = net.engine(ops=ref_ops_fnet3d)
    eng.flat_grad.zero_()
    y, sv = eng.forward(x, torch.float32, True)
    eng.backward(sv, gout)
    return y, {k: eng.g(p).clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("name", ["d2_m4_out1", "d3_m2_out2"])
def test_schedule_matches_statement_autograd(golden, name):
    """the engine's kernel schedule, each op stated in torch, against autograd of the statement: two training steps (running
    statistics carried over), then eval mode"""
    from viscy_amd.unet3d import Unet3d

    case = golden["cases"][name]
    kw = case["kwargs"]
    net = Unet3d(**kw).train()
    net.load_state_dict(case["state_dict"], strict=True)
    ref = ref_fnet3d.FNet3D(**kw).train()
    ref.load_state_dict(case["state_dict"], strict=True)
    g = torch.Generator().manual_seed(7)
    for step in range(2):
        x = case["x"] if step == 0 else torch.randn(case["x"].shape, generator=g)
        gout = case["gout"] if step == 0 else torch.randn(case["gout"].shape, generator=g)
        y, grads = _engine_run(net, x, gout)
        ref.zero_grad()
        yr = ref(x)
        (yr * gout).sum().backward()
        assert _rel(y, yr.detach()) <= 1e-5
        # all gradients together at 1e-5; per tensor at 5e-5 (a 2-channel BatchNorm weight sums thousands of fp32 terms in a
        # different order than autograd does)
        assert _rel(torch.cat([grads[k].flatten() for k, _ in ref.named_parameters()]),
                    torch.cat([p.grad.flatten() for _, p in ref.named_parameters()])) <= 1e-5
        for k, p in ref.named_parameters():
            if k.endswith("proj.bias"):  # feeds a BatchNorm: zero in exact arithmetic, compare against the layer's weight gradient
                scale = dict(ref.named_parameters())[k[:-4] + "weight"].grad.abs().max().item()
                assert grads[k].abs().max().item() <= 1e-5 * scale + 1e-7, k
            else:
                assert _rel(grads[k], p.grad) <= 5e-5, k
        if step == 0:
            for k, v in case["buffers_after"].items():
                assert torch.allclose(net.state_dict()[k].double(), v.double(), rtol=1e-5, atol=1e-7), k
    for k, v in ref.state_dict().items():
        assert torch.allclose(net.state_dict()[k].double(), v.double(), rtol=1e-5, atol=1e-7), k
    net.eval()
    ref.eval()
    with torch.no_grad():
        y, _ = net.engine(ops=ref_ops_fnet3d).forward(case["x"], torch.float32, False)
        assert _rel(y, ref(case["x"])) <= 1e-5
    assert int(net.state_dict()[next(k for k in case["buffers_after"] if "num_batches" in k)]) == 2


def test_guards():
    from viscy_amd.unet3d import Unet3d

    net = Unet3d(depth=3, mult_chan=4)
    with pytest.raises(ValueError, match=r"Spatial dim D=12 must be divisible by 8"):
        net(torch.zeros(1, 1, 12, 16, 16))
    with pytest.raises(ValueError, match=r"Spatial dim W=20 must be divisible by 8"):
        net(torch.zeros(1, 1, 8, 16, 20))
    with pytest.raises(RuntimeError, match="no CPU"):
        net(torch.zeros(1, 1, 8, 16, 16))


def test_vsunet_fnet3d_construction():
    from viscy_amd.losses import MixedLoss
    from viscy_amd.unet3d import Unet3d
    from viscy_amd.vsunet import VSUNet, _make_divisible_pad_amounts

    m = VSUNet(architecture="FNet3D", model_config=dict(in_channels=1, out_channels=1, depth=4, mult_chan=32, in_stack_depth=32))
    assert isinstance(m.model, Unet3d) and m._native
    assert isinstance(m.loss_function, MixedLoss)
    assert tuple(m.example_input_array.shape) == (1, 1, 32, 256, 256)
    assert _make_divisible_pad_amounts((1, 1, 30, 50, 64), 16, True) == [(1, 1), (7, 7), (0, 0)]
    assert _make_divisible_pad_amounts((1, 1, 5, 50, 64), 16, False) == [(0, 0), (7, 7), (0, 0)]
    with pytest.raises(ValueError, match="FNet3D"):
        VSUNet(architecture="2.5D")


def test_fnet3d_recipe_yaml_resolves():
    """the model section of recipes/models/fnet3d.yml through the YAML seam, plus the viscy_models class paths"""
    import yaml

    from viscy_amd import config
    from viscy_amd.unet3d import Unet3d
    from viscy_amd.vsunet import VSUNet

    cfg = yaml.safe_load("""
model:
  class_path: cytoland.engine.VSUNet
  init_args:
    architecture: FNet3D
    model_config:
      in_channels: 1
      out_channels: 1
      depth: 4
      mult_chan: 32
      in_stack_depth: 32
    lr: 0.0002
    schedule: WarmupCosine
""")
    module = config.instantiate(cfg["model"])
    assert isinstance(module, VSUNet) and isinstance(module.model, Unet3d)
    assert module.model.num_blocks == 4 and module.model.out_stack_depth == 32
    for path in ("viscy_models.unet.Unet3d", "viscy_models.unet.unet3d.Unet3d"):
        net = config.instantiate({"class_path": path, "init_args": {"depth": 2, "mult_chan": 4}})
        assert isinstance(net, Unet3d)
