"""CPU: the VSCyto2D model (2x2-stem FullyConvolutionalMAE with the PixelToVoxelShuffleHead) builds with the reference's
state-dict keys and shapes, and the engine's narrow-channel schedule (kernels stated in plain torch: tests/ref_ops_narrow.py)
equals autograd of the oracle — dense fine-tuning (last decoder stage C = 8), masked pre-training (C = 4) and a (5, 2, 2)
Z-stack (narrow stem only)."""

import pytest
import torch

from oracle import fcmae_ref, unext2_ref
from tests import ref_ops_narrow
from viscy_amd.engine_unext2 import Engine
from viscy_amd.fcmae import FullyConvolutionalMAE

FCMAE_2D = dict(in_channels=1, out_channels=2, encoder_blocks=[3, 3, 9, 3], dims=[96, 192, 384, 768], decoder_conv_blocks=2,
                stem_kernel_size=[1, 2, 2], in_stack_depth=1, pretraining=False)  # recipes/models/fcmae_2d.yml
PRETRAIN_2D = dict(FCMAE_2D, out_channels=1, pretraining=True)

SMALL = dict(encoder_blocks=[1, 1, 1, 1], dims=[96, 192, 384, 768], decoder_conv_blocks=1)
CASES = {
    "finetune_c8": (dict(SMALL, in_channels=1, out_channels=2, stem_kernel_size=(1, 2, 2), in_stack_depth=1, pretraining=False),
                    (2, 1, 1, 32, 48), None),
    "pretrain_c4": (dict(SMALL, in_channels=1, out_channels=1, stem_kernel_size=(1, 2, 2), in_stack_depth=1, pretraining=True),
                    (2, 1, 1, 64, 64), 0.5),
    "zstack_522": (dict(SMALL, in_channels=1, out_channels=2, stem_kernel_size=(5, 2, 2), in_stack_depth=5, pretraining=False),
                   (1, 1, 5, 32, 32), None),
}


@pytest.mark.parametrize("kw", [FCMAE_2D, PRETRAIN_2D], ids=["finetune", "pretrain"])
def test_vscyto2d_builds_with_reference_state_dict(kw):
    ref = fcmae_ref.FullyConvolutionalMAE(**kw)
    mine = FullyConvolutionalMAE(**kw)
    rs, ms = ref.state_dict(), mine.state_dict()
    assert list(rs.keys()) == list(ms.keys())
    assert [tuple(v.shape) for v in rs.values()] == [tuple(v.shape) for v in ms.values()]
    mine.load_state_dict(rs, strict=True)
    assert mine.num_blocks == 4 == ref.num_blocks
    assert mine.total_stride == 16
    assert mine.cfg["decoder_channels"][-1] == kw["out_channels"] * 4
    assert mine._core._bf16_ok()


@pytest.mark.parametrize("tag", list(CASES))
def test_vscyto2d_schedule_matches_oracle_autograd(tag):
    kw, shape, ratio = CASES[tag]
    ref = unext2_ref.randomize_(fcmae_ref.FullyConvolutionalMAE(**kw), seed=11)
    mine = FullyConvolutionalMAE(**kw)
    mine.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    masks = None
    mask = None
    if ratio:
        torch.manual_seed(3)
        mask = fcmae_ref.generate_mask(x.shape, mine.total_stride, ratio)
        from viscy_amd.fcmae import stage_row_maps

        kept = mask.shape[-2] * mask.shape[-1] - int(mask.shape[-2] * mask.shape[-1] * ratio)
        h, w = x.shape[-2] // 2, x.shape[-1] // 2
        masks = stage_row_maps(~mask, [(h >> i, w >> i) for i in range(4)], kept)
    ops, calls = _spy()
    eng = Engine(mine._core, ops=ops)
    with torch.no_grad():
        out, sv = eng.forward(x, torch.float32, need_bwd=True, masks=masks)
    y = ref(x, mask=mask) if ratio else ref(x)
    if isinstance(y, tuple):
        y = y[0]
    torch.testing.assert_close(out, y, rtol=2e-4, atol=1e-4 * y.abs().max().item())
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    y.backward(dy)
    with torch.no_grad():
        eng.backward(sv, dy)
    named = dict(mine.named_parameters())
    checked = 0
    for name, p in ref.named_parameters():
        gr = p.grad
        if gr is None or float(gr.abs().max()) == 0.0:
            continue
        gm = eng.g(named[name])
        err = ((gm - gr).abs().max() / gr.abs().max()).item()
        assert err < 2e-3, (name, err)
        checked += 1
    assert checked > 50
    # the narrow branch is what ran
    want = {"narrow_stem_fwd", "narrow_stem_wgrad"}
    if mine.cfg["decoder_channels"][-1] < 16:
        want |= {"narrow_proj_fwd", "narrow_proj_bwd", "narrow_block_fwd1", "narrow_block_fwd2", "narrow_block_bwd_a",
                 "narrow_block_bwd_b", "narrow_block_bwd_c"}
    # (the 4-channel head adjoint is narrow in bf16 only: 4 fp32 channels are one 16-byte vector)
    assert want <= set(calls), sorted(calls)


def _spy():
    """tests.ref_ops_narrow behind a recorder of the narrow_* entry points the engine calls"""
    import types

    calls = {}
    mod = types.ModuleType("tests.ref_ops_narrow_spy")
    for name in dir(ref_ops_narrow):
        f = getattr(ref_ops_narrow, name)
        if name.startswith("narrow_") and callable(f):
            def wrap(*a, _f=f, _n=name, **k):
                calls[_n] = calls.get(_n, 0) + 1
                return _f(*a, **k)
            setattr(mod, name, wrap)
        elif not name.startswith("__"):
            setattr(mod, name, f)
    return mod, calls


def test_oracle_reproduces_reference_golden_2x2():
    """tests/golden/fcmae_2x2.pt (tools/gen_golden_fcmae_2x2.py: the reference's own fcmae.py at the VSCyto2D stems): the oracle
    reproduces output, mask, loss and gradients exactly, and the state-dict keys of the model here are the reference's"""
    from tests.conftest import load_golden

    gold = load_golden("fcmae_2x2.pt")
    assert set(gold) == {"finetune_122", "pretrain_122", "zstack_522"}
    for tag, g in gold.items():
        o = unext2_ref.randomize_(fcmae_ref.FullyConvolutionalMAE(**g["kwargs"]), seed=g["seed"])
        assert list(o.state_dict().keys()) == g["keys"] == list(FullyConvolutionalMAE(**g["kwargs"]).state_dict().keys())
        x = torch.randn(g["x_shape"], generator=torch.Generator().manual_seed(g["x_seed"]))
        if "mask_low" in g:
            y, m = o(x, mask=g["mask_low"])
            loss = fcmae_ref.MaskedMSELoss()(y, x, m)
            assert loss.item() == g["loss"], tag
        else:
            y = o(x)
            loss = (y * torch.randn(y.shape, generator=torch.Generator().manual_seed(g["dy_seed"]))).sum()
        assert torch.equal(y.detach(), g["y"]), tag
        loss.backward()
        named = dict(o.named_parameters())
        for n, gr in g["grads"].items():
            assert ((named[n].grad - gr).abs().max() / gr.abs().max()).item() < 1e-6, (tag, n)


def test_unsupported_narrow_shapes_raise_in_the_constructor():
    with pytest.raises(NotImplementedError, match="12"):  # out_channels 3 -> a 12-channel last stage
        FullyConvolutionalMAE(**dict(FCMAE_2D, out_channels=3))
    with pytest.raises(NotImplementedError, match="in_stack_depth == kz"):
        FullyConvolutionalMAE(**dict(FCMAE_2D, stem_kernel_size=(1, 2, 2), in_stack_depth=3, dims=[96, 192, 384, 768]))


def test_vscyto2d_model_yaml_builds():
    """the model section of the VSCyto2D recipes (recipes/models/fcmae_2d.yml as finetune.yml / predict.yml compose it) through
    the YAML seam"""
    import yaml

    from viscy_amd import config
    from viscy_amd.vsunet import FcmaeUNet

    cfg = yaml.safe_load("""
model:
  class_path: cytoland.engine.FcmaeUNet
  init_args:
    model_config:
      in_channels: 1
      out_channels: 2
      encoder_blocks: [3, 3, 9, 3]
      dims: [96, 192, 384, 768]
      decoder_conv_blocks: 2
      stem_kernel_size: [1, 2, 2]
      in_stack_depth: 1
      pretraining: false
    loss_function:
      class_path: viscy_utils.losses.MixedLoss
      init_args: {l1_alpha: 0.5, l2_alpha: 0.0, ms_dssim_alpha: 0.5}
    lr: 0.0002
    schedule: WarmupCosine
""")
    module = config.instantiate(cfg["model"])
    assert isinstance(module, FcmaeUNet)
    net = module.model
    assert isinstance(net, FullyConvolutionalMAE)
    assert tuple(net.cfg["stem_kernel"]) == (1, 2, 2) and net.num_blocks == 4
    ref = fcmae_ref.FullyConvolutionalMAE(**FCMAE_2D)
    net.load_state_dict(ref.state_dict(), strict=True)


def test_unsupported_2x2_stems_still_raise():
    from viscy_amd.unext2 import UNeXt2

    with pytest.raises(NotImplementedError, match=r"\(k, 4, 4\)"):
        UNeXt2(backbone="convnextv2_atto", stem_kernel_size=(5, 2, 2))
    with pytest.raises(NotImplementedError, match=r"head_conv=False"):
        FullyConvolutionalMAE(**dict(FCMAE_2D, head_conv=True))
