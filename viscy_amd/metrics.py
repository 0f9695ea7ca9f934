"""The metrics of the test stage on MI355X: the names ``cytoland.engine.VSUNet.test_step`` imports from ``torchmetrics.functional``
(applications/cytoland/src/cytoland/engine.py:334-392 of the reference) and ``ssim_25d`` / ``ms_ssim_25d`` of
``viscy_utils.evaluation.metrics`` (metrics.py:272-349) as forward-only metrics.

* ``mean_absolute_error``, ``mean_squared_error``, ``cosine_similarity(reduction="mean")``, ``pearson_corrcoef``, ``r2_score``:
  one ``vsx_pair_sums`` launch each (one read of the pair, every accumulator float64, no atomics), then ``metrics_from_sums`` on the
  thirteen sums; ``regression_metrics`` gives all five from one launch.  Inputs may be non-contiguous views with unit stride along
  X (``x[:, 0, zc:zc + 1]``): they are read in place.
* ``structural_similarity_index_measure``: 4-D input, uniform or Gaussian window up to 33 x 33, on ``vsx_ssim_window``.  The
  library reflect-pads, convolves and crops the padding off again, so what it averages is the windows that lie inside the image;
  the kernel visits exactly those.  It centres both images by their global means before it squares (``E[x^2] - E[x]^2`` in fp32
  loses every digit on fluorescence counts with a large offset), so it is closer to the float64 value than the fp32 library path.
  ``return_full_image`` gives that map of valid windows, ``(B, C, H - Ky + 1, W - Kx + 1)``.
* ``ssim_25d`` / ``ms_ssim_25d``: the per-scale sums of the MixedLoss kernels (``vsx_loss_pool`` / ``vsx_ssim_scale_fwd``, bf16
  rounding points as the reference), combined in torch on the ``[scales][B]`` sums: ``clamp`` and ``betas`` are free here.

Values come back as float64 tensors on the device; nothing synchronises with the host.  No CPU path (``evalkit.device_of``).
"""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from . import ops as O
from ._lib import check, lib, ptr, stream
from .evalkit import device_of

__all__ = ["pair_sums", "metrics_from_sums", "regression_metrics", "mean_absolute_error", "mean_squared_error", "cosine_similarity",
           "pearson_corrcoef", "r2_score", "window_taps", "structural_similarity_index_measure", "ssim_25d", "ms_ssim_25d"]

SUM_NAMES = ("sum_p", "sum_t", "sum_pp", "sum_tt", "sum_pt", "sum_abs", "sum_sq", "min_p", "max_p", "min_t", "max_t", "sum_cos", "rows")
BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ------------------------------------------------------------------------------------------------ host arithmetic
def metrics_from_sums(sums, n) -> dict:
    """The five regression metrics from the thirteen sums of ``vsx_pair_sums`` over ``n`` elements, in float64:
    ``MAE = S|d| / n``, ``MSE = Sd2 / n``, ``cosine = Scos / rows``, ``pearson = C / sqrt(M2p M2t)``, ``r2 = 1 - Sd2 / M2t`` with
    ``M2x = Sxx - Sx^2 / n`` and ``C = Spt - Sp St / n``.  A constant input gives NaN where the definition is 0 / 0.  ``sums`` is a
    sequence or ndarray (-> Python floats) or a float64 tensor (-> 0-dim tensors on its device, no synchronisation)."""
    if torch.is_tensor(sums):
        s = sums.to(torch.float64).unbind(0)
        ctx = None
    else:
        s = np.asarray(sums, dtype=np.float64)
        ctx = np.errstate(invalid="ignore", divide="ignore")
        ctx.__enter__()
    try:
        sp, st, spp, stt, spt, sabs, ssq = (s[i] for i in range(7))
        m2p = spp - sp * sp / n
        m2t = stt - st * st / n
        cov = spt - sp * st / n
        out = {"MAE": sabs / n, "MSE": ssq / n, "cosine": s[11] / s[12], "pearson": cov / (m2p * m2t) ** 0.5, "r2": 1.0 - ssq / m2t}
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return out if torch.is_tensor(sums) else {k: float(v) for k, v in out.items()}


def window_taps(kernel_size: int, sigma: float | None = None) -> np.ndarray:
    """the 1-D window weights in fp32: ``1 / K`` (uniform), or with ``sigma`` the normalised Gaussian ``exp(-(d / sigma)^2 / 2)`` at
    ``d = -(K - 1) / 2 .. (K - 1) / 2`` (torchmetrics' ``_gaussian``, evaluated in fp32 as there)"""
    k = int(kernel_size)
    if sigma is None:
        return np.full(k, np.float32(1.0) / np.float32(k), dtype=np.float32)
    dist = torch.arange((1 - k) / 2, (1 + k) / 2, 1, dtype=torch.float32)
    g = torch.exp(-torch.pow(dist / float(sigma), 2) / 2)
    return (g / g.sum()).numpy()


def gaussian_window_size(sigma: float) -> int:
    """torchmetrics' window for ``gaussian_kernel=True``: ``2 int(3.5 sigma + 0.5) + 1`` whatever ``kernel_size`` says"""
    return 2 * int(3.5 * float(sigma) + 0.5) + 1


# ------------------------------------------------------------------------------------------------ device plumbing
def _planes(x: Tensor, dev: torch.device, name: str) -> tuple[Tensor, int, int, int, int, int]:
    """-> (fp32 tensor on ``dev`` kept alive by the caller, planes, H, W, plane stride, row stride): the leading axes of an at
    least 2-D tensor as one run of planes.  A view is read in place where its X stride is 1 and its leading axes fold into one
    stride; anything else is copied."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    if x.ndim < 2:
        raise ValueError(f"{name} must have at least two axes (..., H, W), got {tuple(x.shape)}")
    x = x.detach().to(device=dev, dtype=torch.float32)
    H, W = int(x.shape[-2]), int(x.shape[-1])
    lead = [(int(n), int(s)) for n, s in zip(x.shape[:-2], x.stride()[:-2]) if n != 1]
    folds = all(a[1] == b[0] * b[1] for a, b in zip(lead, lead[1:]))
    if x.numel() == 0:
        raise ValueError(f"{name} must not be empty, got {tuple(x.shape)}")
    if not (folds and (W == 1 or x.stride(-1) == 1) and min(x.stride()) >= 0):
        x = x.contiguous()
        lead = [(int(n), int(s)) for n, s in zip(x.shape[:-2], x.stride()[:-2]) if n != 1]
    planes = int(np.prod([n for n, _ in lead], dtype=np.int64)) if lead else 1
    plane_stride = lead[-1][1] if lead else 0
    row_stride = int(x.stride(-2)) if H > 1 else W
    return x, planes, H, W, plane_stride, row_stride


def _pair(preds, target, who: str):
    dev = device_of(preds, target, who=who)
    if tuple(preds.shape) != tuple(target.shape):
        raise ValueError(f"preds {tuple(preds.shape)} and target {tuple(target.shape)} must have the same shape")
    p = _planes(preds, dev, "preds")
    t = _planes(target, dev, "target")
    return dev, p, t


def _pair_sums(dev, p, t) -> Tensor:
    (P, planes, H, W, pps, prs), (T, _, _, _, tps, trs) = p, t
    return O.pair_sums(P, (pps, prs), T, (tps, trs), planes, H, W)


def pair_sums(preds, target) -> Tensor:
    """``[VSX_PAIR_SUMS]`` float64 on the device (``SUM_NAMES``): a 1-D input is one row, the leading axes of any other are planes"""
    if getattr(preds, "ndim", 0) == 1:
        preds, target = preds[None], target[None]
    dev, p, t = _pair(preds, target, "metrics")
    return _pair_sums(dev, p, t)


def regression_metrics(preds, target) -> dict[str, Tensor]:
    """``{"MAE", "MSE", "cosine", "pearson", "r2"}`` as 0-dim float64 tensors from one ``vsx_pair_sums`` launch; ``cosine`` is the
    mean over rows along the last axis (``F.cosine_similarity(dim=-1).mean()``), the others are over all elements"""
    s = pair_sums(preds, target)
    return metrics_from_sums(s, int(np.prod(preds.shape, dtype=np.int64)))


def mean_absolute_error(preds, target) -> Tensor:
    return regression_metrics(preds, target)["MAE"]


def mean_squared_error(preds, target) -> Tensor:
    return regression_metrics(preds, target)["MSE"]


def cosine_similarity(preds, target, reduction: str = "mean") -> Tensor:
    """the mean of the cosine similarity of corresponding rows (last axis), as the reference's ``reduction="mean"`` call"""
    if reduction != "mean":
        raise NotImplementedError(f"reduction={reduction!r}: viscy_amd.metrics.cosine_similarity builds the reference's reduction='mean' only")
    return regression_metrics(preds, target)["cosine"]


def pearson_corrcoef(preds, target) -> Tensor:
    """over all elements (the reference flattens both images); its ``* 1e4`` is scale-free in float64 and is not applied"""
    return regression_metrics(preds, target)["pearson"]


def r2_score(preds, target) -> Tensor:
    return regression_metrics(preds, target)["r2"]


# ------------------------------------------------------------------------------------------------ SSIM
_TAPS: dict = {}


def _device_taps(k: int, sigma: float | None, dev) -> Tensor:
    key = (k, sigma, str(dev))
    t = _TAPS.get(key)
    if t is None:
        t = _TAPS[key] = torch.from_numpy(window_taps(k, sigma)).to(dev)
    return t


def _two(v, name: str) -> tuple:
    if isinstance(v, (int, float)):
        return (v, v)
    v = tuple(v)
    if len(v) != 2:
        raise ValueError(f"{name} must be a number or a pair for (B, C, H, W) input, got {v}")
    return v


def ssim_window_sums(dev, p, t, wy: Tensor, wx: Tensor, c: Tensor, shift: Tensor, full: bool = False):
    """``vsx_ssim_window`` on two plane runs of ``_planes`` -> (sums [planes] float64, map [planes, OH, OW] fp32 or None)"""
    (P, planes, H, W, pps, prs), (T, _, _, _, tps, trs) = p, t
    return O.ssim_window(P, (pps, prs), T, (tps, trs), planes, H, W, wy, wx, c, shift, full=full)


def structural_similarity_index_measure(preds, target, gaussian_kernel: bool = True, sigma=1.5, kernel_size=11,
                                        reduction: str | None = "elementwise_mean", data_range=None, k1: float = 0.01, k2: float = 0.03,
                                        return_full_image: bool = False):
    """``torchmetrics.functional.structural_similarity_index_measure`` for ``(B, C, H, W)`` input: per sample the mean of the SSIM
    map over C and the valid windows, then ``reduction`` (``"elementwise_mean"``, ``"sum"``, ``"none"`` / ``None``).
    ``data_range=None`` is ``max(preds.max() - preds.min(), target.max() - target.min())`` over the whole tensors, taken on the
    device from the same ``vsx_pair_sums`` launch that gives the two means the kernel centres by."""
    if preds.ndim == 5:
        raise NotImplementedError("preds: 5-D (B, C, D, H, W) input (torchmetrics' 3-D SSIM) is not built; use ssim_25d for 2.5-D stacks")
    if preds.ndim != 4:
        raise ValueError(f"preds must be (B, C, H, W), got {tuple(preds.shape)}")
    if isinstance(data_range, (tuple, list)):
        raise NotImplementedError("data_range: a (min, max) pair (clamping the inputs) is not built; pass the range as a number or None")
    if reduction not in ("elementwise_mean", "sum", "none", None):
        raise ValueError(f"reduction must be 'elementwise_mean', 'sum', 'none' or None, got {reduction!r}")
    sig = _two(sigma, "sigma")
    if gaussian_kernel:
        if any(s <= 0 for s in sig):
            raise ValueError(f"sigma must be positive, got {sigma}")
        ks = tuple(gaussian_window_size(s) for s in sig)
        what = "sigma"
    else:
        ks = tuple(int(k) for k in _two(kernel_size, "kernel_size"))
        what = "kernel_size"
    if any(k % 2 == 0 or k <= 0 for k in ks):
        raise ValueError(f"kernel_size must be odd and positive, got {kernel_size}")
    if any(k > L.SSIM_MAX_K for k in ks):
        raise NotImplementedError(f"{what}: a {ks[0]} x {ks[1]} window is larger than the kernel's {L.SSIM_MAX_K} x {L.SSIM_MAX_K}")
    if any(k < 3 for k in ks):
        raise NotImplementedError(f"{what}: a {ks[0]} x {ks[1]} window is smaller than 3 x 3")
    dev, p, t = _pair(preds, target, "metrics")
    B, C, H, W = (int(v) for v in preds.shape)
    if H < ks[0] or W < ks[1]:
        raise ValueError(f"kernel_size: a {H} x {W} image holds no {ks[0]} x {ks[1]} window")
    s = _pair_sums(dev, p, t)
    n = float(B * C * H * W)
    if data_range is None:
        dr = torch.maximum(s[8] - s[7], s[10] - s[9])
    else:
        dr = torch.full((), float(data_range), dtype=torch.float64, device=dev)
    c = torch.stack(((k1 * dr) ** 2, (k2 * dr) ** 2)).to(torch.float32)
    shift = (s[0:2] / n).to(torch.float32)
    wy = _device_taps(ks[0], float(sig[0]) if gaussian_kernel else None, dev)
    wx = _device_taps(ks[1], float(sig[1]) if gaussian_kernel else None, dev)
    sums, fmap = ssim_window_sums(dev, p, t, wy, wx, c, shift, full=return_full_image)
    oh, ow = H - ks[0] + 1, W - ks[1] + 1
    per_sample = sums.view(B, C).sum(1) / float(C * oh * ow)
    if reduction == "elementwise_mean":
        val = per_sample.mean()
    elif reduction == "sum":
        val = per_sample.sum()
    else:
        val = per_sample
    if return_full_image:
        return val, fmap.view(B, C, oh, ow)
    return val


# ------------------------------------------------------------------------------------------------ 2.5-D SSIM of the MixedLoss kernels
def _scale_means(preds, target, window, scales: int, who: str) -> tuple[Tensor, Tensor]:
    """-> (ssim, cs), each ``[scales][B]`` float32: the per-sample means of the two maps at every scale of the (1, 2, 2) pyramid"""
    if tuple(window) != (11, 11):
        raise NotImplementedError(f"in_plane_window_size={tuple(window)}: the kernels are built for the reference's default (11, 11)")
    if preds.ndim != 5:
        raise ValueError(f"Input shape must be (B, C, D, W, H), got input shape {tuple(preds.shape)}")
    if tuple(preds.shape) != tuple(target.shape):
        raise ValueError(f"preds {tuple(preds.shape)} and target {tuple(target.shape)} must have the same shape")
    dev = device_of(preds, target, who=who)
    P = preds.detach().to(device=dev, dtype=torch.float32).contiguous()
    T = target.detach().to(device=dev, dtype=torch.float32).contiguous()
    B, C, D, H, W = (int(v) for v in P.shape)
    if (H >> (scales - 1)) < 11 or (W >> (scales - 1)) < 11:
        raise ValueError(f"{scales} scale(s) of the 11 x 11 window need Y, X >= {11 << (scales - 1)} (got {H} x {W})")
    l, s = lib(), stream()
    acc = torch.empty(2 * scales * B, dtype=torch.float32, device=dev)
    tmax = torch.empty(4 * scales, dtype=torch.float32, device=dev)
    check(l.vsx_fill_f32(ptr(acc), acc.numel(), 0.0, s), "fill")
    check(l.vsx_fill_f32(ptr(tmax), tmax.numel(), float("-inf"), s), "fill")
    npix = []
    for sc in range(scales):
        last = sc == scales - 1
        Po = None if last else torch.empty((B, C, D, H // 2, W // 2), dtype=torch.float32, device=dev)
        To = None if last else torch.empty_like(Po)
        tm = tmax[4 * sc: 4 * sc + 4]
        check(l.vsx_loss_pool(ptr(P), ptr(T), ptr(Po), ptr(To), ptr(tm), None, None, B * C * D, H, W, s), "loss_pool")
        check(l.vsx_ssim_scale_fwd(ptr(P), ptr(T), ptr(tm), ptr(acc[sc * B: (sc + 1) * B]),
                                   ptr(acc[(scales + sc) * B: (scales + sc + 1) * B]), B, C, D, H, W, s), "ssim_scale_fwd")
        npix.append(float(C * (H - 10) * (W - 10)))
        if not last:
            P, T, H, W = Po, To, H // 2, W // 2
    means = acc.view(2, scales, B) / torch.tensor(npix, dtype=torch.float32).to(dev).view(1, scales, 1)
    return means[0], means[1]


def ssim_25d(preds, target, in_plane_window_size: tuple[int, int] = (11, 11), return_contrast_sensitivity: bool = False):
    """``viscy_utils.evaluation.metrics.ssim_25d`` (forward only): SSIM per sample ``[B]`` of (B, C, D, H, W) stacks with a uniform
    (D, 11, 11) window and ``target.max()`` as the data range; with ``return_contrast_sensitivity`` also the contrast term"""
    ssim, cs = _scale_means(preds, target, in_plane_window_size, 1, "metrics")
    return (ssim[0], cs[0]) if return_contrast_sensitivity else ssim[0]


def ms_ssim_25d(preds, target, in_plane_window_size: tuple[int, int] = (11, 11), clamp: bool = False,
                betas: Sequence[float] = BETAS) -> Tensor:
    """``viscy_utils.evaluation.metrics.ms_ssim_25d`` (forward only): one scale per entry of ``betas`` (depth is not pooled), the
    contrast term of every scale but the last and the SSIM of the last, optionally clamped at 1e-4, to the power of ``betas``,
    multiplied over the scales and averaged over the batch"""
    betas = tuple(float(b) for b in betas)
    if not betas:
        raise ValueError("betas must not be empty")
    ssim, cs = _scale_means(preds, target, in_plane_window_size, len(betas), "metrics")
    stack = torch.cat((cs[:-1], ssim[-1:]))
    if clamp:
        stack = stack.clamp(min=1e-4)
    b = torch.tensor(betas, dtype=torch.float32).to(stack.device).view(-1, 1)
    return torch.prod(stack ** b, dim=0).mean()
