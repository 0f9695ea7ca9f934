"""SpotlightLoss forward + backward, event-timed, at the bench shape (512 x 2 x 5 x 256 x 256) and the gate shape
(8 x 2 x 5 x 2048 x 2048), for an fp32 and a bf16 prediction, with a uint8 mask, a fixed threshold and Otsu thresholds; achieved
GB/s on the design bytes of DESIGN.md (forward: pred + 4 B target + mask byte; backward: the same + dP).  MixedLoss(0.5, 0, 0.5) at
the bench shape is timed next to it as the only comparison.  SHAPES=bench,gate and REP select."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd.losses import MixedLoss, SpotlightLoss  # noqa: E402

REP = int(os.environ.get("REP", 10))
SHAPES = {"bench": (512, 2, 5, 256, 256), "gate": (8, 2, 5, 2048, 2048)}


def timed(fn, p0, *args, **kw):
    vals = []
    for it in range(REP + 2):
        p = p0.clone().requires_grad_(True)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        loss = fn(p, *args, **kw)
        e1.record()
        loss.backward()
        e2.record()
        torch.cuda.synchronize()
        if it >= 2:
            vals.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
    f = sorted(v[0] for v in vals)[len(vals) // 2]
    b = sorted(v[1] for v in vals)[len(vals) // 2]
    return f, b, loss.item()


for tag in os.environ.get("SHAPES", "bench,gate").split(","):
    shape = SHAPES[tag]
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(shape, device="cuda", generator=g) + 3.0 * (torch.rand(shape, device="cuda", generator=g) < 0.3)
    p32 = t + 0.3 * torch.randn(shape, device="cuda", generator=g)
    mask = (t > 1.5).to(torch.uint8)
    n = t.numel()
    for dt in (torch.float32, torch.bfloat16):
        p0 = p32.to(dt)
        e = p0.element_size()
        for mode, fn, kw, mbytes in (("mask u8", SpotlightLoss(), dict(fg_mask=mask), 1),
                                     ("threshold", SpotlightLoss(fg_threshold=1.5), {}, 0),
                                     ("otsu", SpotlightLoss(), {}, 0)):
            f, b, val = timed(fn, p0, t, **kw)
            fb, bb = n * (e + 4 + mbytes), n * (2 * e + 4 + mbytes)
            if mode == "otsu":
                fb += 2 * n * 4  # the min / max pass and the histogram pass read the target once each
            print(f"{tag} {tuple(shape)} pred {str(dt)[6:]:8s} {mode:9s}: forward {f:.3f} ms ({fb / f / 1e6:.0f} GB/s)  "
                  f"backward {b:.3f} ms ({bb / b / 1e6:.0f} GB/s)  total {f + b:.3f} ms  loss {val:.6f}", flush=True)
    if tag == "bench":
        f, b, val = timed(MixedLoss(0.5, 0.0, 0.5), p32, t)
        print(f"{tag} {tuple(shape)} MixedLoss(0.5, 0, 0.5) fp32: forward {f:.3f} ms  backward {b:.3f} ms  total {f + b:.3f} ms  "
              f"loss {val:.6f}", flush=True)
    del t, p32, mask, p0
    torch.cuda.empty_cache()
