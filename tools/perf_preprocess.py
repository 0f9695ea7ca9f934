"""`viscy preprocess` on the device, timed (profiles/preprocess_perf.txt).

Kernel times are medians of REP runs after WARM untimed ones, HIP events around the call (the launches of a wrapper and its output
allocation included), on
  * one FRAME = Z x H x W uint16 frame resident on the device (default 5 x 2048 x 2048): grid sample at spacing 32 and 8, the 3 x 3
    median with the mask epilogue, the 3 x 3 median of the spacing-8 float32 sample;
  * a SAMPLE of N values (default 10^7), float32 holding uint16 counts: moments pass 1 (integer sums), pass 1 and 2 (float), the four
    vsx_row_select calls behind the seven percentiles, the integer and the 256-bin edge histogram, get_val_stats as a whole.
The median-and-mask kernel is also given as a share of HBM bandwidth on its design bytes, source bytes + 1 byte per pixel, against
the 8.0 TB/s specification and the 6.3 TB/s a float4 copy reaches.
Host yardsticks, timed once in the same run on the same data: scipy.ndimage.median_filter + the comparison on the frame, and
np.nanpercentile / nanmean / nanstd (the reference's get_val_stats) on the sample.
End to end: generate_normalization_metadata + generate_fg_masks on a synthetic uint16 plate (PLATE = positions x T x C x Z x Y x X,
written uncompressed to a temporary directory), the wall clock split into decode (waiting for the host pool), upload, device work
(closed by a synchronise), download and write.

FRAME=5x2048x2048 N=10000000 PLATE=4x2x2x5x1024x1024 REP=20 WARM=3 select."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import preprocess as PP  # noqa: E402

REP = int(os.environ.get("REP", 20))
WARM = int(os.environ.get("WARM", 3))
FRAME = tuple(int(v) for v in os.environ.get("FRAME", "5x2048x2048").split("x"))
N = int(os.environ.get("N", 10_000_000))
PLATE = tuple(int(v) for v in os.environ.get("PLATE", "4x2x2x5x1024x1024").split("x"))
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def timed(fn):
    """(median, fastest, slowest) in ms"""
    torch.cuda.synchronize()
    vals = []
    for it in range(REP + WARM):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            vals.append(e0.elapsed_time(e1))
    vals.sort()
    return vals[len(vals) // 2], vals[0], vals[-1]


def row(name, t, note=""):
    print(f"  {name:<46s} {t[0]:9.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]  {note}", flush=True)


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def frame_part(rng):
    from scipy.ndimage import median_filter

    Z, H, W = FRAME
    host = rng.integers(90, 4000, size=FRAME).astype(np.uint16)
    dev = torch.from_numpy(host).cuda()
    print(f"frame {Z} x {H} x {W} uint16 ({host.nbytes / 1e6:.1f} MB)")
    for g in (32, 8):
        out = torch.empty((Z, -(-H // g), -(-W // g)), device="cuda")
        row(f"vsx_grid_sample g = {g}", timed(lambda: PP.grid_sample(dev, g, out=out)), f"{out.numel()} samples")
    mask = torch.empty(FRAME, dtype=torch.uint8, device="cuda")
    t = timed(lambda: PP.median3x3_mask(dev, 1000.0, out=mask))
    design = host.nbytes + host.size
    row("vsx_median3x3 uint16 -> mask", t, f"{design / 1e6:.1f} MB design bytes: {design / t[0] * 1e3 / 1e12:.2f} TB/s = "
        f"{design / t[0] * 1e3 / HBM_SPEC:.1%} of 8.0 TB/s, {design / t[0] * 1e3 / HBM_COPY:.1%} of the 6.3 TB/s a copy reaches")
    sample = PP.grid_sample(dev, 8)
    smooth = torch.empty_like(sample)
    row("vsx_median3x3 float32 sample (g = 8)", timed(lambda: PP.median3x3(sample, out=smooth)), f"{sample.numel()} values")
    ms, want = host_ms(lambda: (median_filter(host.astype(np.float32), size=(1, 3, 3)) >= 1000.0).astype(np.uint8))
    print(f"  host: astype + scipy median_filter + compare     {ms:9.1f} ms  (one run)")
    assert np.array_equal(mask.cpu().numpy(), want), "device mask differs from scipy's"
    ms, want = host_ms(lambda: median_filter(host[:, ::8, ::8], size=(1, 3, 3)))
    print(f"  host: scipy median_filter of the g = 8 sample    {ms:9.1f} ms  (one run)")
    assert np.array_equal(smooth.cpu().numpy(), want.astype(np.float32))


def sample_part(rng):
    host = rng.integers(90, 4000, size=N).astype(np.uint16)
    x = torch.from_numpy(host.astype(np.float32)).cuda()
    print(f"sample of {N} values (float32 holding uint16 counts, {x.numel() * 4 / 1e6:.1f} MB)")
    t = timed(lambda: PP.nan_moments(x, integral=True))
    row("vsx_nan_moments pass 1, integer sums", t, f"{4 * N / t[0] * 1e3 / 1e12:.2f} TB/s")
    t = timed(lambda: PP.nan_moments(x))
    row("vsx_nan_moments pass 1, float", t, f"{4 * N / t[0] * 1e3 / 1e12:.2f} TB/s")
    t = timed(lambda: PP.nan_moments(x, mean=2000.0))
    row("vsx_nan_moments pass 2", t, f"{4 * N / t[0] * 1e3 / 1e12:.2f} TB/s")
    lo, hi, _ = PP.percentile_ranks(N)
    ranks = sorted(set(lo + hi))
    row(f"vsx_row_select, {len(ranks)} ranks in {-(-len(ranks) // 4)} calls (with the read)", timed(lambda: PP._order_stats(x, lo + hi)))
    row("vsx_hist_int, 3910 bins", timed(lambda: PP.hist_int(x, 90, 3910)))
    xf = x * 0.37
    edges = PP.float_hist_edges(float(xf.min()), float(xf.max()))
    dedges = torch.as_tensor(np.asarray(edges, dtype=np.float64)).cuda()
    counts = torch.empty(256, dtype=torch.int64, device="cuda")

    def hist_edges():
        PP.check(PP.lib().vsx_hist_edges(PP.ptr(xf), N, PP.ptr(dedges), 256, PP.ptr(counts), PP.stream()), "hist_edges")

    row("vsx_hist_edges, 256 bins", timed(hist_edges))
    assert np.array_equal(counts.cpu().numpy(), np.histogram(xf.cpu().numpy(), 256)[0])
    t0 = time.perf_counter()
    for _ in range(5):
        got = PP._val_stats(x, True, np.uint16)
    dev_ms = (time.perf_counter() - t0) / 5 * 1e3
    print(f"  get_val_stats on the device, wall clock           {dev_ms:9.1f} ms  (mean of 5)")
    ms, pct = host_ms(lambda: np.nanpercentile(host, list(PP.PERCENTILES)))
    print(f"  host: np.nanpercentile, seven percentiles         {ms:9.1f} ms  (one run)")
    assert got["p1"] == float(pct[0]) and got["median"] == float(pct[3]) and got["p99"] == float(pct[6])
    ms, _ = host_ms(lambda: (np.nanmin(host), np.nanmax(host), np.nanmean(host), np.nanstd(host)))
    print(f"  host: nanmin / nanmax / nanmean / nanstd          {ms:9.1f} ms  (one run)")


def plate_part(rng):
    from viscy_amd.data import write_hcs_plate

    P, T, C, Z, Y, X = PLATE
    names = [f"ch{c}" for c in range(C)]
    positions = {f"A/{p + 1}/0": rng.integers(90, 4000, size=(T, C, Z, Y, X)).astype(np.uint16) for p in range(P)}
    nbytes = sum(a.nbytes for a in positions.values())
    print(f"plate {P} positions x T {T} x C {C} x Z {Z} x {Y} x {X} uint16 ({nbytes / 1e6:.0f} MB), uncompressed chunks (1, 1, {Z}, {Y}, {X})")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "plate.zarr")
        write_hcs_plate(path, positions, names)
        for label, fn in (("generate_normalization_metadata(32, otsu 8)",
                           lambda tm: PP.generate_normalization_metadata(path, num_workers=8, compute_otsu=True, timings=tm)),
                          (f"generate_fg_masks([{names[-1]}])", lambda tm: PP.generate_fg_masks(path, names[-1:], timings=tm))):
            tm = {}
            t0 = time.perf_counter()
            fn(tm)
            total = time.perf_counter() - t0
            parts = "  ".join(f"{k} {v * 1e3:.0f}" for k, v in tm.items())
            print(f"  {label:<46s} {total * 1e3:9.0f} ms wall:  {parts}  other {1e3 * (total - sum(tm.values())):.0f}  (ms)", flush=True)


def main():
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    print(f"device {torch.cuda.get_device_name(0)}; REP {REP}, WARM {WARM}; median [fastest .. slowest]")
    rng = np.random.default_rng(0)
    frame_part(rng)
    sample_part(rng)
    plate_part(rng)


if __name__ == "__main__":
    main()
