"""SpotlightLoss in float64, written from its formulas, and the case table of tests/test_spotlight_cpu.py and
tests/test_gpu_spotlight.py (tools/gen_golden_spotlight.py runs the same table through the reference).

Per row r = (b, c) of N voxels:
    m    = mask weight (fg_mask as float, else target >= fg_threshold, else target >= otsu[r])
    d    = p - t;  den = k - 2k|p| + 1;  raw = (p - k p) / den;  s = clamp(raw, 0, 1);  s' = (1 - k^2) / den^2 on 0 <= raw <= 1
    F = sum m, Em = sum m d^2, E = sum d^2, S = sum s, I = sum s m
    mse_r = F > 0 ? Em / (F + eps) : E / N;   dice_r = 1 - 2 I / (S + F + eps);   real_r = 0 < F < N
    loss  = lam * mean_r mse_r + (1 - lam) * (n_real > 0 ? sum_r real_r dice_r / n_real : 0)
    dP    = gout * (lam / R * 2 d * (F > 0 ? m / (F + eps) : 1 / N) + (1 - lam) * real_r / n_real * (-2) (m D - I) / D^2 * s'),  D = S + F + eps
"""

import numpy as np
import torch

from viscy_amd._lib import SPOTLIGHT_CHUNK

GRAD_SAMPLE = 512  # the golden keeps at most this many gradient entries per case, evenly strided over the flat gradient


def grad_sample_index(numel: int) -> torch.Tensor:
    step = -(-numel // GRAD_SAMPLE)
    return torch.arange(0, numel, step)


# ------------------------------------------------------------------------------------------------ the arithmetic
def bin_index(x: np.ndarray, lo: np.float32, hi: np.float32, n_bins: int) -> np.ndarray:
    """binning form B: min((int)((x - lo) * n_bins / (hi - lo)), n_bins - 1), every operation rounded to fp32"""
    x = x.astype(np.float32)
    q = ((x - np.float32(lo)) * np.float32(n_bins)) / (np.float32(hi) - np.float32(lo))
    assert q.dtype == np.float32
    return np.minimum(q.astype(np.int64), n_bins - 1)


def otsu_row(x: np.ndarray, n_bins: int = 256) -> np.float32:
    lo, hi = np.float32(x.min()), np.float32(x.max())
    if lo == hi:
        return lo
    h = np.bincount(bin_index(x, lo, hi, n_bins), minlength=n_bins).astype(np.float64)
    w = np.float64(hi) - np.float64(lo)
    centres = np.float64(lo) + ((np.arange(n_bins) + 0.5) * w) / np.float64(n_bins)
    cum_sum, cum_mean = np.cumsum(h), np.cumsum(h * centres)
    total, global_mean = cum_sum[-1], cum_mean[-1]
    mu = cum_mean * total - global_mean * cum_sum
    var = mu * mu / (cum_sum * (total - cum_sum) + 1e-10)
    return np.float32(centres[int(np.argmax(var))])  # np.argmax: the first maximum


def otsu_thresholds(target: torch.Tensor, n_bins: int = 256) -> torch.Tensor:
    B, C = target.shape[:2]
    rows = target.detach().cpu().float().reshape(B * C, -1).numpy()
    return torch.from_numpy(np.array([otsu_row(r, n_bins) for r in rows], dtype=np.float32)).reshape(B, C)


def loss_and_grad(pred, target, fg_mask=None, fg_threshold=None, lambda_mse=0.5, sigmoid_k=-0.95, eps=1e-6, gout=1.0):
    """-> (loss, dP) as float64 tensors, from the values of the inputs as given (pred may hold bf16-rounded values)"""
    B, C = pred.shape[:2]
    R = B * C
    t32 = target.detach().cpu().float().reshape(R, -1)
    p = pred.detach().cpu().double().reshape(R, -1)
    t = t32.double()
    N = p.shape[1]
    if fg_mask is not None:
        m = fg_mask.detach().cpu().double().reshape(R, -1)
    elif fg_threshold is not None:
        m = (t32 >= torch.tensor(fg_threshold, dtype=torch.float32)).double()
    else:
        m = (t32 >= otsu_thresholds(target).reshape(R, 1)).double()
    k, lam = float(sigmoid_k), float(lambda_mse)
    d = p - t
    den = k - 2 * k * p.abs() + 1
    raw = (p - k * p) / den
    s = raw.clamp(0, 1)
    ds = torch.where((raw >= 0) & (raw <= 1), (1 - k * k) / den**2, torch.zeros_like(raw))
    F, Em, E, S, I = m.sum(1), (m * d * d).sum(1), (d * d).sum(1), s.sum(1), (s * m).sum(1)
    has_fg = F > 0
    mse = torch.where(has_fg, Em / (F + eps), E / N)
    D = S + F + eps
    dice = 1 - 2 * I / D
    real = ((F > 0) & (F < N)).double()
    n_real = real.sum()
    dice_term = (real * dice).sum() / n_real if n_real > 0 else torch.zeros((), dtype=torch.float64)
    loss = lam * mse.mean() + (1 - lam) * dice_term
    w_mse = torch.where(has_fg[:, None], m / (F + eps)[:, None], torch.full_like(m, 1.0 / N))
    g = lam / R * 2 * d * w_mse
    if n_real > 0:
        g = g + (1 - lam) * (real / n_real)[:, None] * (-2) * (m * D[:, None] - I[:, None]) / (D * D)[:, None] * ds
    return loss, (gout * g).reshape(pred.shape)


# ------------------------------------------------------------------------------------------------ the cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pair(shape, seed):
    g = _gen(seed)
    target = 0.8 * torch.randn(shape, generator=g) + 0.3
    pred = target + 0.3 * torch.randn(shape, generator=g)
    return g, pred, target


def grid_target(shape, seed, offset=True, constant_last_row=True):
    """targets on the integer grid 0..256 from two separated modes (0-59, 150-256; 30 % high), 0 and 256 present in every row;
    channel c is shifted by 3 c with ``offset``; the last (b, c) row is constant with ``constant_last_row``"""
    g = _gen(seed)
    B, C = shape[:2]
    low = torch.randint(0, 60, shape, generator=g)
    high = torch.randint(150, 257, shape, generator=g)
    t = torch.where(torch.rand(shape, generator=g) < 0.3, high, low).float().reshape(B * C, -1)
    t[:, 0], t[:, 1] = 0.0, 256.0
    if constant_last_row:
        t[-1, :] = 7.0
    t = t.reshape(shape)
    if offset:
        t = t + 3.0 * torch.arange(C, dtype=torch.float32).reshape(1, C, *([1] * (len(shape) - 2)))
    return t


def bimodal_target(shape, seed):
    g = _gen(seed)
    return torch.randn(shape, generator=g) + 3.0 * (torch.rand(shape, generator=g) < 0.3).float()


def _build_random(case):
    g, pred, target = _pair(case["shape"], case["seed"])
    out = dict(pred=pred, target=target, fg_mask=None, fg_threshold=None)
    kind = case["mask"]
    if kind in ("bool", "uint8", "float32"):
        m = torch.rand(case["shape"], generator=g) < 0.4
        out["fg_mask"] = m if kind == "bool" else m.to(getattr(torch, kind))
    elif kind == "thr":
        out["fg_threshold"] = 0.0
    return out


def _build_grid(case):
    target = grid_target(case["shape"], case["seed"])
    g = _gen(case["seed"] + 1)
    pred = torch.where(target > 100, 0.8, 0.1) + 0.3 * torch.randn(case["shape"], generator=g)
    return dict(pred=pred, target=target, fg_mask=None, fg_threshold=None)


def _build_mixed_rows(case):
    """rows: a real mask, all ones, all zeros (unmasked MSE, no Dice), a real mask"""
    g, pred, target = _pair(case["shape"], case["seed"])
    B, C = case["shape"][:2]
    m = (torch.rand(case["shape"], generator=g) < 0.4).reshape(B * C, -1)
    m[1], m[2] = True, False
    return dict(pred=pred, target=target, fg_mask=m.reshape(case["shape"]).to(torch.uint8), fg_threshold=None)


def _build_no_real(case):
    g, pred, target = _pair(case["shape"], case["seed"])
    B, C = case["shape"][:2]
    m = torch.zeros((B * C, pred[0, 0].numel()), dtype=torch.bool)
    m[0] = True
    return dict(pred=pred, target=target, fg_mask=m.reshape(case["shape"]), fg_threshold=None)


def _build_clamp(case):
    """pred holds exact 0 and 1 (the clamp passes a gradient there) and values just outside [0, 1] (it does not)"""
    g, pred, target = _pair(case["shape"], case["seed"])
    flat = pred.reshape(-1)
    if case.get("bf16"):
        ends = [0.0, 1.0, 1.0 + 2.0**-7, -(2.0**-20), 1.0 - 2.0**-8, 2.0**-20]  # neighbours in bf16
    else:
        ends = [0.0, 1.0, 1.0 + 2.0**-10, -1e-30, 1.0 - 2.0**-10, 1e-30]  # raw resolves these from 0 and 1 in fp32 too
    for i, v in enumerate(ends * 4):  # in both channels' rows, masked and unmasked
        flat[10 * i + 2] = v
    m = torch.rand(case["shape"], generator=g) < 0.5
    return dict(pred=pred, target=target, fg_mask=m, fg_threshold=None)


_BUILDERS = {"random": _build_random, "grid": _build_grid, "mixed_rows": _build_mixed_rows, "no_real": _build_no_real,
             "clamp": _build_clamp}

BASE = (2, 2, 5, 32, 32)
ODD = (3, 2, 3, 33, 35)                    # N = 3465: row starts off the 16-byte grid
CHUNK5 = (1, 2, 1, 2 * SPOTLIGHT_CHUNK + 5)  # N = k * CHUNK + 5, k = 2: three workgroups per row, the last one ragged
MULTI = (2, 1, 5, 128, 130)                # N = 83 200: six workgroups per row


def _case(shape, seed, mask, build="random", **kw):
    return dict(shape=tuple(shape), seed=seed, mask=mask, build=build, **kw)


# name -> case.  mask: "bool" / "uint8" / "float32" (fg_mask given), "thr" (fg_threshold = 0.0), "otsu" (neither).
# bf16: pred is rounded to bfloat16 before anything is computed from it.
CASES = {
    "base_bool": _case(BASE, 11, "bool"),
    "base_uint8": _case(BASE, 11, "uint8"),
    "base_float32": _case(BASE, 11, "float32"),
    "base_thr": _case(BASE, 12, "thr"),
    "base_otsu": _case(BASE, 13, "otsu", build="grid"),
    "base_bool_bf16": _case(BASE, 11, "bool", bf16=True),
    "tiny4d_bool": _case((1, 1, 7, 9), 21, "bool"),
    "tiny4d_thr": _case((1, 1, 7, 9), 22, "thr"),
    "odd_bool": _case(ODD, 31, "bool"),
    "odd_float32": _case(ODD, 31, "float32"),
    "odd_thr": _case(ODD, 32, "thr"),
    "odd_otsu": _case(ODD, 33, "otsu", build="grid"),
    "odd_thr_bf16": _case(ODD, 32, "thr", bf16=True),
    "chunk5_bool": _case(CHUNK5, 41, "bool"),
    "chunk5_thr": _case(CHUNK5, 42, "thr"),
    "chunk5_bool_bf16": _case(CHUNK5, 41, "bool", bf16=True),
    "multi_uint8": _case(MULTI, 51, "uint8"),
    "multi_otsu": _case(MULTI, 52, "otsu", build="grid"),
    "mixed_rows": _case((2, 2, 3, 16, 16), 61, "uint8", build="mixed_rows", gout=3.0),
    "no_real": _case((1, 2, 3, 16, 16), 71, "bool", build="no_real"),
    "clamp_ends": _case((1, 2, 1, 8, 16), 81, "bool", build="clamp"),
    "clamp_ends_bf16": _case((1, 2, 1, 8, 16), 81, "bool", build="clamp", bf16=True),
}

# threshold-only cases: name -> (shape, seed, generator)
OTSU_CASES = {
    "grid": ((2, 2, 3, 32, 32), 91, lambda shape, seed: grid_target(shape, seed, offset=False)),
    "grid_multi": (MULTI, 92, lambda shape, seed: grid_target(shape, seed, offset=False, constant_last_row=False)),
    "bimodal": ((2, 2, 5, 64, 64), 93, bimodal_target),
}


def build(name: str) -> dict:
    """CPU tensors of a case: pred, target (float32), fg_mask (or None), fg_threshold (or None), gout"""
    case = CASES[name]
    out = _BUILDERS[case["build"]](case)
    if case.get("bf16"):
        out["pred"] = out["pred"].bfloat16().float()
    out["gout"] = case.get("gout", 1.0)
    return out


def otsu_target(name: str) -> torch.Tensor:
    shape, seed, gen = OTSU_CASES[name]
    return gen(shape, seed)
