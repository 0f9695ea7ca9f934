"""The test stage's metric block, event-timed on the shapes the test stage has: the centre slice of the first channel of a
(B, 2, 5, 2048, 2048) prediction / target pair, B = 1 and B = 8, read in place as ``x[:, 0, 2:3]``.

    python tools/perf_test_metrics.py [--out profiles/test_metrics_perf.txt] [--rep 20]

Per shape: ``vsx_pair_sums``; ``vsx_ssim_window`` for the uniform 21 x 21 and the Gaussian 11 x 11 window; the whole metric block of
``VSUNet.test_step`` (``regression_metrics`` + ``structural_similarity_index_measure``); the plain tensor arithmetic the test step
used before (five metrics, no SSIM) on the same views; and the five-convolution fp32 torch statement of SSIM (what the library
does after its padding) on the device.  Times are medians of ``--rep`` device-event intervals after three warm-up rounds, each
interval around ONE call.  "of HBM" = the bytes the pass must move (both images once, 8 bytes per pixel; outputs are a few hundred
bytes) over the time, against the 8.0 TB/s peak; a float4 copy reaches 6.29 TB/s of it."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import metrics as M  # noqa: E402

PEAK = 8.0e12


def median_ms(fn, rep):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    vals = []
    for _ in range(rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        vals.append(e0.elapsed_time(e1))
    vals.sort()
    return vals[len(vals) // 2], vals[0], vals[-1]


def old_block(p, t):
    """VSUNet.test_step's arithmetic before the kernels"""
    pf, tf = p.flatten(), t.flatten()
    pc, tc = pf - pf.mean(), tf - tf.mean()
    return ((pf - tf).abs().mean(), ((pf - tf) ** 2).mean(), F.cosine_similarity(p, t, dim=-1).mean(),
            (pc * tc).sum() / (pc.norm() * tc.norm()).clamp_min(1e-20), 1 - ((pf - tf) ** 2).sum() / (tc ** 2).sum().clamp_min(1e-20))


def torch_ssim(p, t, w2d, c1, c2):
    """the library's five convolutions in fp32 on the windows inside the image"""
    stack = torch.cat((p, t, p * p, t * t, p * t))
    mp, mt, epp, ett, ept = F.conv2d(stack, w2d).split(p.shape[0])
    vpp, vtt, vpt = (epp - mp * mp).clamp(min=0), (ett - mt * mt).clamp(min=0), ept - mp * mt
    return (((2 * mp * mt + c1) * (2 * vpt + c2)) / ((mp * mp + mt * mt + c1) * (vpp + vtt + c2))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "test_metrics_perf.txt"))
    ap.add_argument("--rep", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_test_metrics needs the MI355X: nothing here is measured without it")
    dev = torch.device("cuda")
    lines = [f"test-stage metric block, {torch.cuda.get_device_name(0)}, medians of {args.rep} device-event intervals (min .. max)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    S = args.size
    for B in (1, 8):
        g = torch.Generator(device="cuda").manual_seed(B)
        target = torch.rand((B, 2, 5, S, S), device=dev, generator=g) * 3 + 100
        pred = target + 0.3 * torch.randn(target.shape, device=dev, generator=g)
        p, t = pred[:, 0, 2:3], target[:, 0, 2:3]
        n = p.numel()
        need = 8.0 * n
        say(f"-- B = {B}: {n} pixels per image, {need / 1e6:.1f} MB to read once")
        _, pp, tp = M._pair(p, t, "metrics")
        sums = M._pair_sums(dev, pp, tp)
        c = torch.stack(((0.01 * 3.0) ** 2 * torch.ones((), device=dev), (0.03 * 3.0) ** 2 * torch.ones((), device=dev))).float()
        shift = (sums[0:2] / n).float()

        def row(name, fn, bytes_needed=None):
            med, lo, hi = median_ms(fn, args.rep)
            tail = f"  {bytes_needed / (med * 1e-3) / 1e9:7.1f} GB/s = {100 * bytes_needed / (med * 1e-3) / PEAK:5.1f} % of HBM" if bytes_needed else ""
            say(f"{name:58s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f}){tail}")
            return med

        row("vsx_pair_sums", lambda: M._pair_sums(dev, pp, tp), need)
        for label, k, sigma in (("uniform 21 x 21", 21, None), ("Gaussian 11 x 11", 11, 1.5)):
            w = M._device_taps(k, sigma, dev)
            row(f"vsx_ssim_window, {label}", lambda w=w: M.ssim_window_sums(dev, pp, tp, w, w, c, shift), need)
        new = row("test_step metric block: regression_metrics + SSIM(21)",
                  lambda: (M.regression_metrics(p, t), M.structural_similarity_index_measure(p, t, gaussian_kernel=False, kernel_size=21)),
                  2 * need)
        old = row("previous test_step arithmetic (five metrics, no SSIM)", lambda: old_block(p, t))
        w2d = torch.full((1, 1, 21, 21), 1.0 / 441, device=dev)
        pc, tc = p.contiguous(), t.contiguous()
        conv = row("torch fp32 SSIM, five 21 x 21 convolutions", lambda: torch_ssim(pc, tc, w2d, c[0], c[1]))
        say(f"   five metrics + SSIM on the kernels / five metrics in tensor arithmetic: {new / old:.3f}")
        say(f"   five metrics + SSIM on the kernels / (tensor arithmetic + torch SSIM): {new / (old + conv):.3f}")
        del pred, target, p, t, pc, tc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
