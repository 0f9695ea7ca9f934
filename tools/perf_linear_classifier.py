"""LogisticRegression on the device, event-timed: the three passes of a Newton iteration (vsx_logreg_rows, vsx_wcolsum with
{r, s}, vsx_gram_scaled), the margins-only pass of decision_function, and ``LogisticRegression(solver="liblinear",
class_weight="balanced", max_iter=1000).fit`` end to end (upload of the host array not included: the embeddings are on the device),
for N x d embeddings with two classes at 1:3.  Yardsticks: vsx_col_moments over the same bytes for the two bandwidth passes, and
sklearn's liblinear on the host CPU on the same data (one run in a child process, given up after SKLEARN_LIMIT seconds).

The data are drawn on the host with torch's seeded CPU generator (class means 3 apart along a random direction, unit noise), so a
host without a device draws the same rows: DEVICE=0 runs the sklearn yardstick alone.
SHAPES=100000x768,1000000x768 REP=3 SKLEARN=1 SKLEARN_MAX_N=1000000 SKLEARN_LIMIT=600 select."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REP = int(os.environ.get("REP", 3))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "100000x768,1000000x768").split(",")]
PARAMS = dict(solver="liblinear", class_weight="balanced", max_iter=1000)
SCRATCH = os.environ.get("SCRATCH", tempfile.gettempdir())   # the device part leaves its coefficients here for the sklearn child


def draw(n, d):
    """-> (x float32 (n, d) host tensor, y int64 (n,)): a quarter of the rows are class 1"""
    g = torch.Generator().manual_seed(n + d)
    y = (torch.rand(n, generator=g) < 0.25).to(torch.int64)
    direction = torch.randn(d, generator=g)
    direction *= 1.5 / direction.norm()
    x = torch.empty(n, d)
    for r0 in range(0, n, 1 << 16):
        m = min(1 << 16, n - r0)
        x[r0:r0 + m] = torch.randn(m, d, generator=g) + (2.0 * y[r0:r0 + m, None].float() - 1.0) * direction
    return x, y.numpy()


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


def device_part(n, d, x_host, y):
    from viscy_amd import ops
    from viscy_amd.linear_classifier import LogisticRegression

    x = x_host.cuda()
    labels = torch.from_numpy(y.astype(np.int32)).cuda()
    w = (0.05 * torch.randn(d, dtype=torch.float64, generator=torch.Generator().manual_seed(1))).cuda()
    cp, cn = n / (2.0 * y.sum()), n / (2.0 * (n - y.sum()))
    t_mom, _ = timed(lambda: ops.col_moments(x))
    t_rows, out = timed(lambda: ops.logreg_rows(x, w, 0.1, labels, 1, cp, cn))
    t_trial, _ = timed(lambda: ops.logreg_rows(x, w, 0.1, labels, 1, cp, cn, derivatives=False))
    t_marg, _ = timed(lambda: ops.logreg_margins(x, w, 0.1))
    t_wcs, _ = timed(lambda: ops.wcolsum(x, out["rs"]))
    t_gram, _ = timed(lambda: ops.gram_scaled(x, out["q"]))
    gb = n * d * 4 / 1e9
    tiles, rps = -(-d // 128), ops.gram_rows_per_split(n, d)
    print(f"(N, d) = ({n}, {d}), classes {n - int(y.sum())} : {int(y.sum())}, balanced\n"
          f"  col_moments (yardstick) {t_mom:.2f} ms = {2 * gb / t_mom:.2f} TB/s over its two passes\n"
          f"  logreg_rows {t_rows:.2f} ms = {gb / t_rows:.2f} TB/s (z, r, s, q and the sums);  sums alone (a line-search trial) {t_trial:.2f} ms = "
          f"{gb / t_trial:.2f} TB/s;  margins alone {t_marg:.2f} ms = {gb / t_marg:.2f} TB/s\n"
          f"  wcolsum m=2 {t_wcs:.2f} ms = {gb / t_wcs:.2f} TB/s\n"
          f"  gram_scaled {t_gram:.2f} ms = {n * d * (d + 128.0) / t_gram / 1e9:.1f} TFLOP/s ({tiles * (tiles + 1) // 2} tile pairs x "
          f"{-(-n // rps)} splits of {rps} rows)", flush=True)
    est = LogisticRegression(**PARAMS)
    est.fit(x, y)   # warm-up: allocator, first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est = LogisticRegression(**PARAMS).fit(x, y)
    torch.cuda.synchronize()
    t_fit = (time.perf_counter() - t0) * 1e3
    info = est.fit_info_[0]
    passes = (info.n_iter + 1) * (t_rows + t_wcs + t_gram) + info.n_evals * t_trial
    print(f"  fit end to end {t_fit:.0f} ms: {info.n_iter} Newton iterations, {info.n_evals} line-search evaluations, |g| / |g(0)| = "
          f"{info.grad_norm / info.grad_norm0:.1e}; the device passes are {passes:.0f} ms of it, the rest is the host ((d + 1)^2 Cholesky, copies "
          f"of the Gram)", flush=True)
    np.save(os.path.join(SCRATCH, f"perf_logreg_coef_{n}x{d}.npy"), np.concatenate((est.coef_[0], est.intercept_)))
    return est


def sklearn_child(n, d):
    """one liblinear fit on the host; prints its time and writes the coefficients"""
    from sklearn.linear_model import LogisticRegression as SkLR

    x, y = draw(n, d)
    xh = x.numpy()
    t0 = time.perf_counter()
    sk = SkLR(**PARAMS).fit(xh, y)
    t = time.perf_counter() - t0
    path = os.path.join(SCRATCH, f"perf_logreg_coef_{n}x{d}.npy")
    note = ""
    if os.path.exists(path):
        u = np.load(path)
        note = f"; |[coef; intercept] - the device's| = {np.linalg.norm(np.concatenate((sk.coef_[0], sk.intercept_)) - u):.2e} of {np.linalg.norm(u):.2f}"
    print(f"  sklearn liblinear on the host (one thread, one run, tol 1e-4): {t:.1f} s, n_iter_ {int(sk.n_iter_[0])}{note}", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--sklearn-child":
        return sklearn_child(int(sys.argv[2]), int(sys.argv[3]))
    device = bool(int(os.environ.get("DEVICE", 1)))
    want_sk = bool(int(os.environ.get("SKLEARN", 1)))
    max_n, limit = int(os.environ.get("SKLEARN_MAX_N", 1000000)), float(os.environ.get("SKLEARN_LIMIT", 600))
    for n, d in SHAPES:
        if device:
            x, y = draw(n, d)
            device_part(n, d, x, y)
            del x
            torch.cuda.empty_cache()
        else:
            print(f"(N, d) = ({n}, {d})")
        if not want_sk:
            continue
        if n > max_n:
            print(f"  sklearn liblinear on the host: not run at this size (SKLEARN_MAX_N={max_n})", flush=True)
            continue
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--sklearn-child", str(n), str(d)], timeout=limit, check=True)
        except subprocess.TimeoutExpired:
            print(f"  sklearn liblinear on the host: one run did not finish in {limit:.0f} s", flush=True)


if __name__ == "__main__":
    main()
