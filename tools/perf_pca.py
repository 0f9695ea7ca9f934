"""PCA on the device, event-timed: the three kernels of csrc/pca.hip (vsx_col_moments, vsx_gram_centered, vsx_center_project), the
host part (viscy_amd.reduce.pca_from_moments: float64 scaling, eigh, flip) and compute_pca end to end (upload of a host array not
included: the embeddings of `predict` are on the device), for N x d embeddings, k in K and both normalize_features settings.
Yardstick: the reference's route on the host CPU (sklearn StandardScaler -> PCA(n_components, random_state=42), float32, the
host's threads, one run, copy of the data from the device not counted), where sklearn is importable.

The Gram pass is reported as a fraction of its own floor, the larger of
  bytes of X once at the HBM rate            N d 4 B / 8.0 TB/s
  N d (d + 128) flop at the f32-MFMA rate    / 157.3 TFLOP/s     (upper-triangular 128 x 128 tiles: (d^2 + 128 d) / 2 products)
both peaks as MI355X_MICROARCH.md gives them (spec).  The data are the planted-spectrum rows of tests/ref_pca.py drawn on the
device.  SHAPES=100000x768,1000000x768 K=8,50 REP=3 SKLEARN=1 select."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import ops  # noqa: E402
from viscy_amd import reduce as R  # noqa: E402

REP = int(os.environ.get("REP", 3))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "100000x768,1000000x768").split(",")]
KS = [int(v) for v in os.environ.get("K", "8,50").split(",")]
HBM, MFMA_F32 = 8.0e12, 157.3e12


def timed(fn, rep=REP):
    """median device time in ms after one warm-up run, and the last result"""
    torch.cuda.synchronize()
    vals = []
    for it in range(rep + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            vals.append(e0.elapsed_time(e1))
    return sorted(vals)[len(vals) // 2], out


def host_timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def planted(n, d, seed):
    """offset + eight planted directions (variances 64 .. 0.5) + an isotropic floor, as tests/ref_pca.py, drawn on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(d, 8, device="cuda", generator=g))
    s = 8.0 * (0.5 ** 0.5) ** torch.arange(8, device="cuda")
    x = torch.empty(n, d, device="cuda")
    for r0 in range(0, n, 1 << 17):   # in slabs: no second N x d buffer
        m = min(1 << 17, n - r0)
        x[r0:r0 + m] = (torch.randn(m, 8, device="cuda", generator=g) * s) @ q.T + 0.1 * torch.randn(m, d, device="cuda", generator=g)
    x += (torch.rand(d, device="cuda", generator=g) * 2 - 1) * 80.0
    return x


def main():
    try:
        import sklearn
        from sklearn.decomposition import PCA as SkPCA
        from sklearn.preprocessing import StandardScaler as SkScaler
        have_sklearn = bool(int(os.environ.get("SKLEARN", 1)))
    except ImportError:
        have_sklearn = False
        print("sklearn is not importable on this host: no CPU yardstick")
    for n, d in SHAPES:
        x = planted(n, d, n)
        t_mom, (mean, m2) = timed(lambda: ops.col_moments(x))
        t_gram, gram = timed(lambda: ops.gram_centered(x, mean))
        floor_b, floor_f = n * d * 4 / HBM * 1e3, n * d * (d + 128.0) / MFMA_F32 * 1e3
        floor = max(floor_b, floor_f)
        tiles, rps = -(-d // 128), ops.gram_rows_per_split(n, d)
        print(f"(N, d) = ({n}, {d}):  gram plan {tiles * (tiles + 1) // 2} tile pairs x {-(-n // rps)} splits of {rps} rows, workspace "
              f"{ops.lib().vsx_gram_ws_bytes(n, d) / 2 ** 20:.0f} MiB\n"
              f"  col_moments {t_mom:.2f} ms = {2 * n * d * 4 / t_mom / 1e9:.2f} TB/s over its two passes\n"
              f"  gram_centered {t_gram:.2f} ms = {n * d * (d + 128.0) / t_gram / 1e9:.1f} TFLOP/s; floor {floor:.2f} ms "
              f"({'flop' if floor_f >= floor_b else 'bytes'}-bound: bytes {floor_b:.2f} ms, flop {floor_f:.2f} ms): {floor / t_gram:.1%} of its floor",
              flush=True)
        mh, m2h, gh = mean.cpu().numpy(), m2.cpu().numpy(), gram.cpu().numpy()
        for normalize in (True, False):
            for k in KS:
                t_host, fit = host_timed(lambda: R.pca_from_moments(n, mh, m2h, gh, k, normalize))
                w = torch.from_numpy(fit.projection_weights()).cuda()
                t_proj, z = timed(lambda: ops.center_project(x, mean, w))
                t0 = time.perf_counter()
                pc, _ = R.compute_pca(x, n_components=k, normalize_features=normalize)
                t_all = (time.perf_counter() - t0) * 1e3
                print(f"  normalize_features={normalize!s:5s} k={k:3d}: host eigh + attributes {t_host:.1f} ms, center_project {t_proj:.2f} ms "
                      f"= {2.0 * n * d * k / t_proj / 1e9:.1f} TFLOP/s ({n * (d + k) * 4 / t_proj / 1e9:.2f} TB/s), compute_pca end to end "
                      f"{t_all:.1f} ms (copy of the (N, k) result and the DataFrame included)", flush=True)
        if have_sklearn:
            xh = x.cpu().numpy()
            for normalize in (True, False):
                t0 = time.perf_counter()
                feats = SkScaler().fit_transform(xh) if normalize else xh
                est = SkPCA(n_components=KS[0], random_state=42)
                zs = est.fit_transform(feats)
                t_sk = (time.perf_counter() - t0) * 1e3
                pc, _ = R.compute_pca(x, n_components=KS[0], normalize_features=normalize)
                sg = np.sign((pc[:1000].astype(np.float64) * zs[:1000]).sum(0))
                diff = float(np.abs(pc * sg - zs).max() / np.abs(zs).max())
                print(f"  sklearn {sklearn.__version__} on the host ({os.environ.get('OMP_NUM_THREADS', '?')} threads, one run, solver "
                      f"{est._fit_svd_solver}) normalize_features={normalize!s:5s} k={KS[0]}: {t_sk:.0f} ms; max |Z - Z_sklearn| / max |Z| {diff:.2e}",
                      flush=True)
            del xh
        del x, gram
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
