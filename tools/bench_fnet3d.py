"""FNet3D (recipes/models/fnet3d.yml: depth 4, mult_chan 32, 1 -> 1 channel) on one MI355X: prints one JSON line with

  * the training step at the recipe shape (B = 24, 32 x 64 x 64; MSE, the VSUNet default; AdamW; hipGraph-captured) in bf16 and
    in fp32: ms and patches / s, and the achieved TFLOP/s against the forward count of 76.1 GFLOP per patch (a step = 3x);
  * the same step of the plain-torch statement (tests/ref_fnet3d.py, eager under autocast(bf16), MIOpen convolutions, torch
    AdamW) on the same GPU, as the yardstick;
  * a Z-32 predict of one 512 x 512 field of view (bf16, eval, captured).

    python tools/bench_fnet3d.py [--batch 24] [--steps 10] [--fov 512]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(in_channels=1, out_channels=1, depth=4, mult_chan=32)


def fwd_flops(depth=4, mult=32, cin=1, cout=1, shape=(32, 64, 64)) -> float:
    """multiply-adds x 2 of one forward per patch (convolutions and transposed convolutions; BatchNorm / ReLU not counted)"""
    dims = [mult * 2 ** i for i in range(depth + 1)]
    vox = [shape[0] * shape[1] * shape[2] / 8 ** l for l in range(depth + 1)]
    f = vox[0] * 27 * cin * dims[0] + vox[0] * 27 * dims[0] * cout
    for l in range(depth):
        f += vox[l] * 27 * dims[l] * dims[l] * 2                    # encoder block
        f += vox[l + 1] * 27 * dims[l] * dims[l + 1]                # downsample
        f += vox[l] * 27 * (2 * dims[l] * dims[l] + dims[l] * dims[l])  # decoder block
        f += vox[l + 1] * 27 * dims[l + 1] * dims[l]                # transposed conv (as a dense 2x grid / 8 parity classes)
    f += vox[depth] * 27 * dims[depth] * dims[depth] * 2            # bottleneck
    return 2 * f


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
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--fov", type=int, default=512)
    a = ap.parse_args()
    from tests.ref_fnet3d import FNet3D
    from viscy_amd.losses import MixedLoss
    from viscy_amd.optim import FlatAdamW
    from viscy_amd.step import InferStep, TrainStep
    from viscy_amd.unet3d import Unet3d

    dev = torch.device("cuda:0")
    B = a.batch
    g = torch.Generator().manual_seed(7)
    x = torch.randn((B, 1, 32, 64, 64), generator=g).to(dev)
    tgt = torch.randn((B, 1, 32, 64, 64), generator=g).to(dev)
    gf = fwd_flops()
    rec = {"workload": f"FNet3D depth 4 mult 32, B={B}, 32x64x64, MSE, AdamW, hipGraph", "fwd_gflop_per_patch": round(gf / 1e9, 1)}
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        torch.manual_seed(42)
        m = Unet3d(**KW).to(dev).train()
        m.compute_dtype, m.grad_mode = dt, "flat"
        step = TrainStep(m, MixedLoss(0.0, 1.0, 0.0), FlatAdamW(m.engine(), lr=1e-4), None, use_graph=True, static_inputs=True)
        ms, loss = _time(lambda: step(x, tgt), a.steps)
        rec.update({f"{name}_ms_per_step": round(ms, 2), f"{name}_patches_per_s": round(B / ms * 1e3, 1),
                    f"{name}_tflops": round(3 * gf * B / ms / 1e9, 1), f"{name}_loss": round(float(loss), 5)})
        del step, m
        torch.cuda.empty_cache()

    torch.manual_seed(42)
    ref = FNet3D(**KW).to(dev).train()
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-4)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ref(x)
        loss = torch.nn.functional.mse_loss(y.float(), tgt)
        loss.backward()
        opt.step()
        return loss

    ms, loss = _time(torch_step, a.steps)
    rec.update(torch_autocast_ms_per_step=round(ms, 2), torch_autocast_patches_per_s=round(B / ms * 1e3, 1),
               torch_autocast_tflops=round(3 * gf * B / ms / 1e9, 1))
    del ref, opt
    torch.cuda.empty_cache()

    torch.manual_seed(42)
    m = Unet3d(**KW).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    fov = torch.randn((1, 1, 32, a.fov, a.fov), generator=g).to(dev)
    inf = InferStep(m, use_graph=True)
    ms, y = _time(lambda: inf(fov), max(a.steps // 2, 3))
    rec.update(predict_fov=f"32x{a.fov}x{a.fov}", predict_ms=round(ms, 2), predict_finite=bool(torch.isfinite(y).all().item()))
    rec["bf16_vs_torch"] = round(rec["torch_autocast_ms_per_step"] / rec["bf16_ms_per_step"], 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
