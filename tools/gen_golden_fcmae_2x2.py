"""Writes tests/golden/fcmae_2x2.pt: the reference's own FullyConvolutionalMAE (viscy_models/unet/fcmae.py, executed on the
stubbed timm / monai modules of oracle/validate_against_reference.py) at the 2x2 stems of the VSCyto2D recipes, checked
EXACTLY against oracle/fcmae_ref.py before anything is written:

  * ``finetune_122``: recipes/models/fcmae_2d.yml widths (in 1, out 2, blocks 3-3-9-3, dims 96..768, 2 decoder blocks),
    stem (1, 2, 2), in_stack_depth 1 (the Conv2d stem branch), 64 x 96 input, dense forward + a fixed upstream gradient;
  * ``pretrain_122``: the same widths with out_channels 1, masked pre-training at ratio 0.5 with the reference's own mask
    draw (torch.manual_seed(5)), MaskedMSELoss;
  * ``zstack_522``: a small (5, 2, 2) Z-stack model (conv3d stem, K = 20).

Each entry holds the constructor kwargs, the oracle seed (unext2_ref.randomize_), the input seed / shape, the output, the
mask (low resolution), the loss and the gradients of a few parameters.

    python tools/gen_golden_fcmae_2x2.py [--out tests/golden/fcmae_2x2.pt]

Needs the reference tree the validation module points at (REF); the other G-fixtures are regenerated into a scratch
directory on the way (their setup installs the stubs) and thrown away.
"""

from __future__ import annotations

import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEEP = ["encoder.stem.conv2d.weight", "encoder.stem.conv3d.weight", "encoder.stem.norm.weight", "encoder.stages.0.blocks.0.dwconv.weight",
        "encoder.stages.3.blocks.0.mlp.grn.weight", "decoder.decoder_stages.2.conv.downsample.1.weight",
        "decoder.decoder_stages.2.conv.blocks.0.mlp.fc1.weight", "decoder.decoder_stages.2.conv.blocks.0.mlp.grn.weight",
        "decoder.decoder_stages.2.conv.blocks.1.dwconv.weight", "decoder.decoder_stages.2.conv.blocks.1.mlp.fc2.weight"]

FCMAE_2D = dict(in_channels=1, out_channels=2, encoder_blocks=[3, 3, 9, 3], dims=[96, 192, 384, 768], decoder_conv_blocks=2,
                stem_kernel_size=[1, 2, 2], in_stack_depth=1, pretraining=False)
CASES = [
    ("finetune_122", FCMAE_2D, (2, 1, 1, 64, 96), None),
    ("pretrain_122", dict(FCMAE_2D, out_channels=1, pretraining=True), (2, 1, 1, 64, 96), 0.5),
    ("zstack_522", dict(in_channels=1, out_channels=2, encoder_blocks=[1, 1, 2, 1], dims=[96, 192, 384, 768], decoder_conv_blocks=1,
                        stem_kernel_size=[5, 2, 2], in_stack_depth=5, pretraining=False), (2, 1, 5, 32, 48), None),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fcmae_2x2.pt"))
    a = ap.parse_args()
    torch.set_num_threads(8)
    from oracle import fcmae_ref as F
    from oracle import unext2_ref as R
    from oracle import validate_against_reference as V

    V.GOLD = tempfile.mkdtemp()  # the stub setup below also writes its own fixtures: not into tests/golden
    V.g8_wiring()
    V.g9_fcmae()
    ref = sys.modules["viscy_models.unet.fcmae"]
    golden = {}
    for tag, kw, shape, ratio in CASES:
        r = ref.FullyConvolutionalMAE(**kw)
        o = F.FullyConvolutionalMAE(**kw)
        assert list(r.state_dict().keys()) == list(o.state_dict().keys()), tag
        assert [tuple(v.shape) for v in r.state_dict().values()] == [tuple(v.shape) for v in o.state_dict().values()], tag
        R.randomize_(o, seed=21)
        r.load_state_dict(o.state_dict(), strict=True)
        x = torch.randn(shape, generator=torch.Generator().manual_seed(51))
        ent = {"kwargs": kw, "seed": 21, "x_seed": 51, "x_shape": shape, "keys": list(o.state_dict().keys())}
        if ratio:
            torch.manual_seed(5)
            yr, mask_r = r(x, mask_ratio=ratio)
            stride = r.encoder.total_stride
            low = mask_r[:, :, ::stride, ::stride].clone()
            yo, mask_o = o(x, mask=low)
            assert stride == 16 and torch.equal(mask_o, mask_r), tag
            lr_ = F.MaskedMSELoss()(yr, x, mask_r)
            lo = F.MaskedMSELoss()(yo, x, mask_o)
            ent.update(mask_ratio=ratio, mask_low=low, loss=lr_.item())
            assert lo.item() == lr_.item(), tag
        else:
            yr, yo = r(x), o(x)
            dy = torch.randn(yr.shape, generator=torch.Generator().manual_seed(52))
            lr_, lo = (yr * dy).sum(), (yo * dy).sum()
            ent.update(dy_seed=52)
        assert V.maxrel(yo, yr) == 0.0, tag
        lr_.backward()
        lo.backward()
        gr, go = dict(r.named_parameters()), dict(o.named_parameters())
        keep = [n for n in KEEP if n in gr and gr[n].grad is not None]
        for n in keep:
            assert V.maxrel(go[n].grad, gr[n].grad) < 1e-6, (tag, n)
        ent.update(y=yr.detach().clone(), grads={n: gr[n].grad.clone() for n in keep})
        golden[tag] = ent
        print(f"fcmae 2x2 {tag}: reference == oracle (exact forward{', mask, loss' if ratio else ''}); {len(keep)} gradients kept")
    torch.save(golden, a.out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
