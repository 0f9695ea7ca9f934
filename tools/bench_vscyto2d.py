"""VSCyto2D (2x2-stem FCMAE, recipes/models/fcmae_2d.yml widths) on one MI355X: prints one JSON line with

  * the fine-tune training step (B = 32, 256 x 256, bf16, MixedLoss, AdamW at lr 0, hipGraph-captured): ms and patches / s;
  * the pre-training step (out_channels = 1, mask ratio 0.5, MaskedMSELoss, same capture);
  * predict of one 2048 x 2048 field of view (bf16, forward only, captured).

    python tools/bench_vscyto2d.py [--batch 32] [--size 256] [--steps 20] [--fov 2048]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FCMAE_2D = dict(in_channels=1, out_channels=2, encoder_blocks=[3, 3, 9, 3], dims=[96, 192, 384, 768], decoder_conv_blocks=2,
                stem_kernel_size=[1, 2, 2], in_stack_depth=1, pretraining=False)


def _model(kw, dev):
    from viscy_amd.fcmae import FullyConvolutionalMAE

    torch.manual_seed(42)
    m = FullyConvolutionalMAE(**kw).to(dev)
    m.compute_dtype, m.grad_mode = torch.bfloat16, "flat"
    return m


def _time(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--fov", type=int, default=2048)
    a = ap.parse_args()
    from viscy_amd.losses import MaskedMSELoss, MixedLoss
    from viscy_amd.optim import FlatAdamW
    from viscy_amd.step import InferStep, TrainStep

    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    g = torch.Generator().manual_seed(7)
    x = torch.randn((B, 1, 1, S, S), generator=g).to(dev)
    tgt = torch.rand((B, 2, 1, S, S), generator=g).to(dev)
    rec = {"workload": f"VSCyto2D FCMAE (1,2,2) fcmae_2d widths, B={B}, {S}x{S}, bf16, hipGraph, AdamW lr 0"}

    m = _model(FCMAE_2D, dev)
    step = TrainStep(m, MixedLoss(0.5, 0.0, 0.5), FlatAdamW(m.engine(), lr=0.0), None, use_graph=True, static_inputs=True)
    ms, loss = _time(lambda: step(x, tgt), a.steps)
    rec.update(finetune_ms_per_step=round(ms, 3), finetune_patches_per_s=round(B / ms * 1e3, 1), finetune_loss=round(float(loss), 5))
    del step, m

    m = _model(dict(FCMAE_2D, out_channels=1, pretraining=True), dev)
    crit = MaskedMSELoss()

    def pre_loss(xx, _t):  # a fresh device-side mask draw per step (graph-capturable)
        y, mk = m(xx, mask_ratio=0.5)
        return crit(y, xx, mk)

    step = TrainStep(m, None, FlatAdamW(m.engine(), lr=0.0), None, use_graph=True, loss_fn=pre_loss, static_inputs=True)
    ms, loss = _time(lambda: step(x, x), a.steps)
    rec.update(pretrain_ms_per_step=round(ms, 3), pretrain_loss=round(float(loss), 5))
    del step, m

    m = _model(FCMAE_2D, dev).eval()
    fov = torch.randn((1, 1, 1, a.fov, a.fov), generator=g).to(dev)
    inf = InferStep(m, use_graph=True)
    ms, y = _time(lambda: inf(fov), max(a.steps // 4, 3))
    rec.update(predict_fov=a.fov, predict_ms=round(ms, 3), predict_finite=bool(torch.isfinite(y).all().item()))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
