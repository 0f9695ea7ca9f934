"""Float64 restatements, case tables, bounds and runners for the test-stage kernels (csrc/test_metrics.hip) and their Python layer
(viscy_amd/metrics.py).  tests/test_metrics_cpu.py checks the restatements against scipy / sklearn / numpy and against the two
padded readings of the library's SSIM; tests/test_gpu_test_metrics.py runs the kernels against them.

Bounds are counted, not chosen.  With u64 = 2^-53, u32 = 2^-24:

* a float64 sum whose every term passes through at most ``depth`` additions is within ``depth * u64 * sum |terms|`` of the exact
  sum; ``pair_depth`` / ``ssim_fold_depth`` count the additions of the kernels' fixed summation orders from the exported launch
  constants.  The exact sums of the reference side are ``math.fsum`` (correctly rounded), so the whole bound belongs to the kernel.
* ``metric_bounds`` carries the sums' bounds through ``metrics_from_sums`` to first order (the partial derivatives of the five
  expressions, plus 4 u64 of each intermediate for the host arithmetic itself) and refuses data on which first order is not enough.
* ``ssim_formula64`` evaluates the SSIM formula in float64 next to a running bound for the kernel's fp32 evaluation of it: every
  fp32 operation after the five window means adds ``u32 |result|`` to the error carried by its operands (products and the quotient
  by the usual first-order rules with the second-order terms kept).  In the exact cases the window means themselves carry no
  error: dyadic taps on small integers are exact in fp32 in any order.
"""

from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from viscy_amd import _lib as L

U64, U32 = 2.0 ** -53, 2.0 ** -24
F32, F64 = torch.float32, torch.float64
NAN, SENT, GUARD = float("nan"), 77.0, 64
TS = L.SSIM_TILE
WAVES, VEC, MAX_WGS, NQ = L.PAIR_SUMS_WAVES, L.PAIR_SUMS_VEC, L.PAIR_SUMS_MAX_WGS, L.PAIR_SUMS
FOLD_SEGS_PAIR, FOLD_SEGS_SSIM = 16, 256  # the runs the two fold kernels cut their lists into (csrc/test_metrics.hip)
EXACT_Q = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12)  # every quantity but the cosine sum is an integer on integer images


# ------------------------------------------------------------------------------------------------ regression metrics, float64
def exact_sums(p: np.ndarray, t: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """-> (the thirteen quantities of vsx_pair_sums, the sums of the terms' magnitudes) for [planes, H, W] fp32 arrays: products and
    differences of fp32 values are exact in float64 and math.fsum rounds each sum once.  The cosine entry is the fsum of the rows'
    float64 cosines."""
    p64, t64 = p.astype(np.float64).reshape(-1, p.shape[-1]), t.astype(np.float64).reshape(-1, t.shape[-1])
    d = p64 - t64
    fs = lambda a: math.fsum(a.ravel().tolist())  # noqa: E731
    pn = np.array([math.sqrt(fs(r * r)) for r in p64])
    tn = np.array([math.sqrt(fs(r * r)) for r in t64])
    cos = np.array([fs(a * b) for a, b in zip(p64, t64)]) / (np.maximum(pn, 1e-8) * np.maximum(tn, 1e-8))
    s = np.array([fs(p64), fs(t64), fs(p64 * p64), fs(t64 * t64), fs(p64 * t64), fs(np.abs(d)), fs(d * d), p64.min(), p64.max(),
                  t64.min(), t64.max(), fs(cos), float(p64.shape[0])])
    mag = np.array([fs(np.abs(p64)), fs(np.abs(t64)), s[2], s[3], fs(np.abs(p64 * t64)), s[5], s[6], 0, 0, 0, 0, fs(np.abs(cos)), 0])
    return s, mag


def regression64(p: np.ndarray, t: np.ndarray) -> dict:
    """the five metrics by their definitions on centred float64 data (two passes, no E[x^2] - E[x]^2)"""
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    d = (p64 - t64).ravel()
    pc, tc = p64.ravel() - p64.mean(), t64.ravel() - t64.mean()
    rows_p, rows_t = p64.reshape(-1, p.shape[-1]), t64.reshape(-1, t.shape[-1])
    cos = (rows_p * rows_t).sum(1) / (np.maximum(np.sqrt((rows_p ** 2).sum(1)), 1e-8) * np.maximum(np.sqrt((rows_t ** 2).sum(1)), 1e-8))
    return {"MAE": float(np.abs(d).mean()), "MSE": float((d * d).mean()), "cosine": float(cos.mean()),
            "pearson": float((pc * tc).sum() / math.sqrt((pc * pc).sum() * (tc * tc).sum())),
            "r2": float(1.0 - (d * d).sum() / (tc * tc).sum())}


def pair_launch(planes: int, H: int) -> tuple[int, int]:
    """(workgroups, rows a wave takes at most) of vsx_pair_sums: a function of planes * H alone"""
    rows = planes * H
    wgs = min(-(-rows // WAVES), MAX_WGS)
    return wgs, -(-rows // (wgs * WAVES))


def pair_depth(planes: int, H: int, W: int) -> tuple[int, int]:
    """-> (additions a term of the seven element sums passes through at most, the same for a term of one row's three sums).  A lane
    takes at most VEC * ceil(W / (64 VEC)) + 1 elements of a row (vector loads, then the scalar tail; the scalar path takes fewer)
    and adds all its rows' elements into one accumulator; then 6 butterfly steps, the workgroup's waves, the fold's run and runs."""
    wgs, rows_per_wave = pair_launch(planes, H)
    per_lane = VEC * -(-W // (64 * VEC)) + 1
    tail = 6 + (WAVES - 1) + -(-wgs // FOLD_SEGS_PAIR) + (FOLD_SEGS_PAIR - 1)
    return rows_per_wave * per_lane + tail, per_lane + 6


def sum_bounds(p: np.ndarray, t: np.ndarray, s: np.ndarray, mag: np.ndarray) -> np.ndarray:
    """the bound of each of the thirteen device quantities against ``exact_sums``"""
    planes, H, W = p.shape
    depth, row_depth = pair_depth(planes, H, W)
    e = depth * U64 * mag
    e[[7, 8, 9, 10, 12]] = 0.0
    # a row's cosine: pt within row_depth u64 sum |p t|, each norm within (row_depth / 2 + 1) u64 of itself, then a product, a
    # quotient and two max: 4 u64 |cos|; the rows' cosines are then summed like any other term (rows_per_wave additions in a wave)
    p64, t64 = p.astype(np.float64).reshape(-1, W), t.astype(np.float64).reshape(-1, W)
    pn = np.maximum(np.sqrt((p64 * p64).sum(1)), 1e-8)
    tn = np.maximum(np.sqrt((t64 * t64).sum(1)), 1e-8)
    cos = (p64 * t64).sum(1) / (pn * tn)
    per_row = row_depth * U64 * np.abs(p64 * t64).sum(1) / (pn * tn) + (row_depth + 2 + 4) * U64 * np.abs(cos)
    e[11] = per_row.sum() * (1 + 1e-6) + (pair_launch(planes, H)[1] + depth) * U64 * np.abs(cos).sum()
    return e


def metric_bounds(s: np.ndarray, e: np.ndarray, n: int) -> dict:
    """first-order bounds of metrics_from_sums(s', n) - metrics_from_sums(s, n) for |s' - s| <= e, host arithmetic included"""
    sp, st, spp, stt, spt, sabs, ssq = s[:7]
    m2p, m2t, cov = spp - sp * sp / n, stt - st * st / n, spt - sp * st / n
    e_m2p = e[2] + 2 * abs(sp) * e[0] / n + e[0] ** 2 / n + 4 * U64 * (abs(spp) + sp * sp / n)
    e_m2t = e[3] + 2 * abs(st) * e[1] / n + e[1] ** 2 / n + 4 * U64 * (abs(stt) + st * st / n)
    e_cov = e[4] + (abs(sp) * e[1] + abs(st) * e[0] + e[0] * e[1]) / n + 4 * U64 * (abs(spt) + abs(sp * st) / n)
    assert e_m2p <= 1e-3 * m2p and e_m2t <= 1e-3 * m2t, "the data are too close to constant for a first-order bound"
    r = cov / math.sqrt(m2p * m2t)
    r2 = 1.0 - ssq / m2t
    grow = 1.002  # what first order leaves out while the relative errors stay below 1e-3
    return {"MAE": e[5] / n + 4 * U64 * sabs / n, "MSE": e[6] / n + 4 * U64 * ssq / n, "cosine": e[11] / s[12] + 4 * U64 * abs(s[11] / s[12]),
            "pearson": grow * (e_cov / math.sqrt(m2p * m2t) + abs(r) * 0.5 * (e_m2p / m2p + e_m2t / m2t)) + 4 * U64 * abs(r),
            "r2": grow * (e[6] / m2t + ssq / m2t * e_m2t / m2t) + 4 * U64 * (1 + abs(r2))}


# ------------------------------------------------------------------------------------------------ SSIM, float64 and the fp32 library path
def window2d(wy: np.ndarray, wx: np.ndarray, dtype) -> torch.Tensor:
    return torch.outer(torch.from_numpy(np.asarray(wy)).to(dtype), torch.from_numpy(np.asarray(wx)).to(dtype))


def window_means64(P: torch.Tensor, T: torch.Tensor, wy, wx, sp: float, st: float):
    """the five weighted means over every window inside [planes, H, W] float64 images, of x = p - sp, y = t - st"""
    w = window2d(wy, wx, F64)[None, None]
    x, y = (P.to(F64) - sp)[:, None], (T.to(F64) - st)[:, None]
    return [F.conv2d(v, w)[:, 0] for v in (x, y, x * x, y * y, x * y)]


def ssim_formula64(mx, my, exx, eyy, exy, sp: float, st: float, c1: float, c2: float):
    """-> (SSIM in float64, the bound of the kernel's fp32 evaluation of the same formula on the same means)"""
    u = U32
    a_ = lambda v: v.abs()  # noqa: E731

    def mul(a, ea, b, eb):
        v = a * b
        return v, a_(a) * eb + a_(b) * ea + ea * eb + u * a_(v)

    def add(a, ea, b, eb):
        v = a + b
        return v, ea + eb + u * a_(v)

    zero = torch.zeros_like(mx)
    mxx, e_mxx = mul(mx, zero, mx, zero)
    myy, e_myy = mul(my, zero, my, zero)
    mxy, e_mxy = mul(mx, zero, my, zero)
    vxx, e_vxx = add(exx, zero, -mxx, e_mxx)
    vyy, e_vyy = add(eyy, zero, -myy, e_myy)
    vxy, e_vxy = add(exy, zero, -mxy, e_mxy)
    vxx, vyy = vxx.clamp_min(0), vyy.clamp_min(0)  # max(., 0) moves a value by no more than its error
    cst = lambda v: torch.full_like(mx, float(v))  # noqa: E731
    mp, e_mp = add(mx, zero, cst(sp), zero)
    mt, e_mt = add(my, zero, cst(st), zero)
    a, e_a = mul(mp, e_mp, mt, e_mt)
    pp, e_pp = mul(mp, e_mp, mp, e_mp)
    tt, e_tt = mul(mt, e_mt, mt, e_mt)
    n1, e_n1 = add(2 * a, 2 * e_a, cst(c1), zero)
    n2, e_n2 = add(2 * vxy, 2 * e_vxy, cst(c2), zero)
    num, e_num = mul(n1, e_n1, n2, e_n2)
    s1, e_s1 = add(pp, e_pp, tt, e_tt)
    d1, e_d1 = add(s1, e_s1, cst(c1), zero)
    s2, e_s2 = add(vxx, e_vxx, vyy, e_vyy)
    d2, e_d2 = add(s2, e_s2, cst(c2), zero)
    den, e_den = mul(d1, e_d1, d2, e_d2)
    q = num / den
    assert bool((a_(den) > 2 * e_den).all()), "a denominator is not separated from zero"
    return q, (e_num + a_(q) * e_den) / (a_(den) - e_den) + u * a_(q)


def ssim_valid64(P, T, wy, wx, c1: float, c2: float, with_bound: bool = False, sp=None, st=None):
    """the SSIM map over the windows inside the planes, float64 ([planes, H - Ky + 1, W - Kx + 1]); centred by the global means
    unless a shift is given (the value does not depend on it; the fp32 bound does)"""
    P, T = torch.as_tensor(P).to(F64), torch.as_tensor(T).to(F64)
    sp = float(P.mean()) if sp is None else float(sp)
    st = float(T.mean()) if st is None else float(st)
    q, bound = ssim_formula64(*window_means64(P, T, wy, wx, sp, st), sp, st, c1, c2)
    return (q, bound) if with_bound else q


def ssim_padded64(P, T, K: int, pad: int, c1: float, c2: float):
    """the library's route for a uniform K x K window, float64: reflect-pad by ``pad``, convolve without padding, crop ``pad`` off
    the map.  pad = (K - 1) / 2 is the newer library's reading, pad = 5 (from the Gaussian size, whatever kernel_size is) the older
    one's.  No centring: float64 needs none."""
    P, T = torch.as_tensor(P).to(F64)[:, None], torch.as_tensor(T).to(F64)[:, None]
    Pp, Tp = F.pad(P, (pad,) * 4, mode="reflect"), F.pad(T, (pad,) * 4, mode="reflect")
    w = torch.full((1, 1, K, K), 1.0 / (K * K), dtype=F64)
    mp, mt, epp, ett, ept = [F.conv2d(v, w) for v in (Pp, Tp, Pp * Pp, Tp * Tp, Pp * Tp)]
    vpp, vtt, vpt = (epp - mp * mp).clamp_min(0), (ett - mt * mt).clamp_min(0), ept - mp * mt
    full = ((2 * mp * mt + c1) * (2 * vpt + c2)) / ((mp * mp + mt * mt + c1) * (vpp + vtt + c2))
    return full[:, 0, pad:full.shape[2] - pad, pad:full.shape[3] - pad]


def ssim_library_fp32(P32: torch.Tensor, T32: torch.Tensor, wy, wx, c1: float, c2: float) -> torch.Tensor:
    """the five-convolution statement of the library in fp32 torch on the windows inside the planes: the yardstick of the real-valued
    tests, run on the CPU"""
    w = window2d(wy, wx, F32)[None, None]
    p, t = P32.to(F32)[:, None], T32.to(F32)[:, None]
    stack = torch.cat((p, t, p * p, t * t, p * t))
    mp, mt, epp, ett, ept = F.conv2d(stack, w).split(p.shape[0])
    mpp, mtt, mpt = mp.pow(2), mt.pow(2), mp * mt
    vpp, vtt, vpt = (epp - mpp).clamp(min=0.0), (ett - mtt).clamp(min=0.0), ept - mpt
    upper, lower = 2 * vpt + c2, vpp + vtt + c2
    return (((2 * mpt + c1) * upper) / ((mpp + mtt + c1) * lower))[:, 0]


def ssim_fold_depth(oh: int, ow: int) -> int:
    """additions a map value passes through at most on its way into the plane's sum: 2 per half tile in a thread, the 8 levels of
    the workgroup's tree, the fold's run over the plane's tiles and its 8 levels"""
    tiles = -(-oh // TS) * -(-ow // TS)
    return 4 + 8 + -(-tiles // FOLD_SEGS_SSIM) + 8


def c_of(dr: float, k1: float = 0.01, k2: float = 0.03) -> tuple[float, float]:
    """c1, c2 as the fp32 values the kernel reads"""
    return float(np.float32((k1 * dr) ** 2)), float(np.float32((k2 * dr) ** 2))


def dyadic_taps(k: int, phase: int = 0) -> np.ndarray:
    """k taps that are powers of two and sum to exactly 1: with 2^(e-1) < k <= 2^e, 2^e - k taps of 2^-(e-1) (from position
    ``phase`` on, cyclically) and 2 k - 2^e of 2^-e.  Any sum of products of two of them with integers below 64 is exact in fp32
    whatever its order (terms with at most 12 fractional bits, sums below 2^12).  A sum of 1 makes the window means means: the
    value does not depend on the shift and E[x^2] >= E[x]^2"""
    e = max(1, math.ceil(math.log2(k)))
    big = 2 ** e - k
    taps = np.full(k, 2.0 ** -e, dtype=np.float32)
    taps[[(phase + i) % k for i in range(big)]] = 2.0 ** -(e - 1)
    assert float(taps.astype(np.float64).sum()) == 1.0
    return taps


# ------------------------------------------------------------------------------------------------ case tables
def _pc(name, planes, H, W, rs=None, ps=None, off=0):
    rs = W if rs is None else rs
    return {"name": name, "planes": planes, "H": H, "W": W, "rs": rs, "ps": H * rs if ps is None else ps, "off": off}


def pair_cases() -> list[dict]:
    """shapes of vsx_pair_sums: strides in elements, ``off`` = the first element's offset from a 256-byte aligned address"""
    full = 64 * VEC  # elements of a row one pass of a wave's vector loads covers; the loop takes two passes at a time while it can
    cases = [_pc("1x1x1", 1, 1, 1), _pc("w1", 2, 5, 1), _pc("w_odd", 1, 3, 37)]
    cases += [_pc(f"w{w}", 1, 2, w) for w in (VEC - 1, VEC, VEC + 1, full - 1, full, full + 1, 2 * full - 1, 2 * full, 2 * full + 1)]
    cases += [_pc(f"h{h}", 1, h, 8) for h in (WAVES - 1, WAVES, WAVES + 1)]
    cases += [_pc("planes3", 3, 5, 12), _pc("row_stride", 2, 4, 20, rs=28), _pc("plane_stride_odd", 3, 4, 16, ps=4 * 16 + 3),
              _pc("unaligned_base", 1, 3, 24, off=1), _pc("unaligned_tail", 2, 3, 2 * full + 7, rs=2 * full + 12, off=4),
              _pc("centre_slice_view", 2, 24, 40, ps=2 * 5 * 24 * 40, off=2 * 24 * 40),
              _pc("past_the_grid", 1, WAVES * MAX_WGS + 9, 3), _pc("past_the_grid_twice", 2, WAVES * MAX_WGS + 1, 5)]
    return cases


def real_pair_cases() -> list[dict]:
    keep = ("w_odd", f"w{64 * VEC + 1}", "row_stride", "plane_stride_odd", "unaligned_tail", "past_the_grid")
    return [dict(c, offset=o, name=f"{c['name']}-offset{o}") for c in pair_cases() if c["name"] in keep for o in (0, 1000)]


def _sc(name, oh, ow, ky, kx=None, planes=1, rs_pad=0, ps_pad=0):
    kx = ky if kx is None else kx
    H, W = oh + ky - 1, ow + kx - 1
    rs = W + rs_pad
    return {"name": name, "planes": planes, "H": H, "W": W, "Ky": ky, "Kx": kx, "rs": rs, "ps": H * rs + ps_pad, "off": 0}


def ssim_exact_cases() -> list[dict]:
    """output extents 1, TS - 1, TS, TS + 1, 2 TS + 1 on either axis (and the half tile's 15 / 16 / 17 rows), every window size,
    Ky != Kx, an odd W under a longer row stride, three planes under a plane stride that leaves the rows unaligned"""
    cases = [_sc(f"k3_{oh}x{ow}", oh, ow, 3) for oh, ow in ((1, 1), (TS - 1, TS + 1), (TS, TS), (TS + 1, TS - 1), (2 * TS + 1, 2 * TS + 1),
                                                           (1, 2 * TS + 1), (2 * TS + 1, 1), (TS // 2 - 1, TS // 2 + 1), (TS // 2, TS),
                                                           (TS // 2 + 1, TS // 2 - 1))]
    cases += [_sc(f"k{k}_{oh}x{ow}", oh, ow, k) for k in (11, 21, 33) for oh, ow in ((1, 1), (TS + 1, TS - 1))]
    cases += [_sc("k33_65x33", 2 * TS + 1, TS + 1, 33), _sc("k5x11_33x20", TS + 1, 20, 5, 11), _sc("k21x7_9x40", 9, 40, 21, 7),
              _sc("k11_w_odd_row_stride", 20, 25, 11, rs_pad=6), _sc("k11_planes3", TS + 2, TS - 3, 11, planes=3, rs_pad=1, ps_pad=5),
              _sc("k3_planes3", 5, 2 * TS + 3, 3, planes=3)]
    return cases


def ssim_real_cases() -> list[dict]:
    """uniform 21 and Gaussian 11 (sigma 1.5), 64 x 64 up to 150 x 150"""
    out = []
    for kind, k in (("uniform", 21), ("gaussian", 11)):
        for H, W in ((64, 64), (101, 150), (150, 150)):
            out.append({"name": f"{kind}{k}_{H}x{W}", "kind": kind, "K": k, "H": H, "W": W})
    return out


REAL_OFFSETS = (0.0, 100.0, 1000.0)


def real_taps(case) -> np.ndarray:
    from viscy_amd.metrics import window_taps

    return window_taps(case["K"], 1.5 if case["kind"] == "gaussian" else None)


def real_images(case, offset: float, seed: int = 11) -> tuple[torch.Tensor, torch.Tensor]:
    """target = uniform * 3 + offset, pred = target + 0.3 N(0, 1): the same noise at every offset, fp32, [1, H, W]"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((1, case["H"], case["W"]), generator=g, dtype=F64) * 3
    noise = 0.3 * torch.randn((1, case["H"], case["W"]), generator=g, dtype=F64)
    t = (base + offset).to(F32)
    return (base + offset + noise).to(F32), t


_FIX: dict = {}


def real_fixture(case) -> dict:
    """per offset the images, c, the float64 map; and the yardstick: the fp32 library statement's own error at offset 0"""
    key = ("real", case["name"])
    if key not in _FIX:
        wy = wx = real_taps(case)
        fx = {"taps": wy, "offsets": {}}
        for off in REAL_OFFSETS:
            p, t = real_images(case, off)
            dr = max(float(p.max()) - float(p.min()), float(t.max()) - float(t.min()))
            c1, c2 = c_of(dr)
            fx["offsets"][off] = {"p": p, "t": t, "c": (c1, c2), "map64": ssim_valid64(p, t, wy, wx, c1, c2)}
        o0 = fx["offsets"][0.0]
        lib32 = ssim_library_fp32(o0["p"], o0["t"], wy, wx, *o0["c"]).to(F64)
        fx["yard_max"] = float((lib32 - o0["map64"]).abs().max())
        fx["yard_mean"] = abs(float(lib32.mean()) - float(o0["map64"].mean()))
        _FIX[key] = fx
    return _FIX[key]


def clear_fixtures() -> None:
    _FIX.clear()


# ------------------------------------------------------------------------------------------------ buffers
class Poisoned:
    """an input of ``planes`` x H x W fp32 values at the case's strides inside a NaN-filled buffer (GUARD NaN before and after, NaN
    in every gap between rows and planes): a read outside the image turns a sum into NaN"""

    def __init__(self, values: torch.Tensor, case: dict, dev):
        planes, H, W, rs, ps, off = (case[k] for k in ("planes", "H", "W", "rs", "ps", "off"))
        span = (planes - 1) * ps + (H - 1) * rs + W
        start = 64 + off  # torch allocations are 256-byte aligned: the image starts ``off`` elements past such an address
        self.buf = torch.full((start + span + GUARD,), NAN, dtype=F32)
        view = self.buf.as_strided((planes, H, W), (ps, rs, 1), start)
        view.copy_(values.reshape(planes, H, W))
        self.buf = self.buf.to(dev)
        self.t = self.buf.as_strided((planes, H, W), (ps, rs, 1), start)
        self.ps, self.rs = ps, rs

    def ptr(self) -> int:
        return self.t.data_ptr()


class Guarded:
    """an output between two sentinel-filled guards that starts as NaN"""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.fill_(NAN)

    def check(self, what: str):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).double().cpu()
        assert bool((g == SENT).all()), f"{what}: a guard element next to the output was written"
        assert not bool(self.t.isnan().any()), f"{what}: {int(self.t.isnan().sum())} of {self.t.numel()} elements are NaN"
        return self.t

    def untouched(self) -> bool:
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).double().cpu()
        return bool((g == SENT).all()) and bool(self.t.isnan().all())


class LibEntry:
    """the two C-ABI entry points with workspaces of exactly the size the library asks for, NaN-filled between guards"""

    def __init__(self, lib):
        self.lib = lib

    def err(self) -> str:
        return self.lib.vsx_last_error().decode(errors="replace")

    def pair_sums(self, P: Poisoned, T: Poisoned, case, dev) -> torch.Tensor:
        planes, H, W = case["planes"], case["H"], case["W"]
        need = self.lib.vsx_pair_sums_ws_bytes(planes, H)
        assert need == pair_launch(planes, H)[0] * NQ * 8, (need, pair_launch(planes, H))
        ws, out = Guarded((need // 8,), F64, dev), Guarded((NQ,), F64, dev)
        rc = self.lib.vsx_pair_sums(P.ptr(), P.ps, P.rs, T.ptr(), T.ps, T.rs, planes, H, W, out.t.data_ptr(), ws.t.data_ptr(), need,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.err()
        torch.cuda.synchronize()
        ws.check(f"{case['name']}: workspace")  # every partial the grid owns was written
        return out.check(f"{case['name']}: sums").cpu()

    def ssim(self, P: Poisoned, T: Poisoned, case, wy, wx, c, shift, dev, full=True):
        planes, H, W, ky, kx = (case[k] for k in ("planes", "H", "W", "Ky", "Kx"))
        oh, ow = H - ky + 1, W - kx + 1
        need = self.lib.vsx_ssim_window_ws_bytes(planes, H, W, ky, kx)
        assert need == planes * -(-oh // TS) * -(-ow // TS) * 8, need
        ws, sums = Guarded((need // 8,), F64, dev), Guarded((planes,), F64, dev)
        fmap = Guarded((planes, oh, ow), F32, dev) if full else None
        dv = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(dev)  # noqa: E731
        wy_d, wx_d, c_d, s_d = dv(wy), dv(wx), dv(c), dv(shift)
        rc = self.lib.vsx_ssim_window(P.ptr(), P.ps, P.rs, T.ptr(), T.ps, T.rs, planes, H, W, wy_d.data_ptr(), ky, wx_d.data_ptr(), kx,
                                      c_d.data_ptr(), s_d.data_ptr(), sums.t.data_ptr(), fmap.t.data_ptr() if full else None, ws.t.data_ptr(),
                                      need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.err()
        torch.cuda.synchronize()
        ws.check(f"{case['name']}: workspace")
        return sums.check(f"{case['name']}: sums").cpu(), (fmap.check(f"{case['name']}: map").cpu() if full else None)


# ------------------------------------------------------------------------------------------------ runners (GPU)
MARGINS: dict = {}  # worst observed error / bound per check, printed by the GPU file's last test


def _note(what: str, ratio: float) -> None:
    MARGINS[what] = max(MARGINS.get(what, 0.0), float(ratio))
    print(f"margin {what}: {ratio:.3g}")


def integer_pair(case, seed: int = 3) -> tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed + case["planes"] * 7 + case["H"] * 3 + case["W"])
    shape = (case["planes"], case["H"], case["W"])
    return (torch.randint(-8, 9, shape, generator=g).to(F32), torch.randint(-8, 9, shape, generator=g).to(F32))


def run_pair_exact(ep: LibEntry, case, dev) -> None:
    """integer images: every sum is an exact float64 -> sums, extrema and the row count bit-equal to int64 arithmetic, twice"""
    p, t = integer_pair(case)
    pi, ti = p.numpy().astype(np.int64), t.numpy().astype(np.int64)
    d = pi - ti
    want = {0: pi.sum(), 1: ti.sum(), 2: (pi * pi).sum(), 3: (ti * ti).sum(), 4: (pi * ti).sum(), 5: np.abs(d).sum(), 6: (d * d).sum(),
            7: pi.min(), 8: pi.max(), 9: ti.min(), 10: ti.max(), 12: pi.shape[0] * pi.shape[1]}
    P, T = Poisoned(p, case, dev), Poisoned(t, case, dev)
    got = ep.pair_sums(P, T, case, dev)
    for q in EXACT_Q:
        assert got[q].item() == float(want[q]), (case["name"], q, got[q].item(), int(want[q]))
    s, mag = exact_sums(p.numpy(), t.numpy())
    e = sum_bounds(p.numpy(), t.numpy(), s, mag)
    assert abs(got[11].item() - s[11]) <= e[11], (case["name"], "cosine", got[11].item(), s[11], e[11])
    _note("pair_sums cosine sum (integer images)", abs(got[11].item() - s[11]) / max(e[11], 1e-300))
    again = ep.pair_sums(P, T, case, dev)
    assert torch.equal(got, again), (case["name"], "two runs differ", got, again)


def run_pair_real(ep: LibEntry, case, dev) -> None:
    g = torch.Generator().manual_seed(5)
    shape = (case["planes"], case["H"], case["W"])
    t = (torch.randn(shape, generator=g, dtype=F64) + case["offset"]).to(F32)
    p = (t.to(F64) + 0.3 * torch.randn(shape, generator=g, dtype=F64)).to(F32)
    s, mag = exact_sums(p.numpy(), t.numpy())
    e = sum_bounds(p.numpy(), t.numpy(), s, mag)
    got = ep.pair_sums(Poisoned(p, case, dev), Poisoned(t, case, dev), case, dev).numpy()
    for q in range(NQ):
        assert abs(got[q] - s[q]) <= e[q], (case["name"], q, got[q], s[q], e[q])
        if e[q] > 0:
            _note(f"pair_sums {q}", abs(got[q] - s[q]) / e[q])
    from viscy_amd.metrics import metrics_from_sums

    n = p.numel()
    have, want, bound = metrics_from_sums(got, n), metrics_from_sums(s, n), metric_bounds(s, e, n)
    for k in want:
        assert abs(have[k] - want[k]) <= bound[k], (case["name"], k, have[k], want[k], bound[k])
        _note(f"metrics_from_sums {k}", abs(have[k] - want[k]) / bound[k])


def integer_images(case, seed: int = 9) -> tuple[torch.Tensor, torch.Tensor]:
    """values 0 .. 7, different in every plane"""
    g = torch.Generator().manual_seed(seed + case["H"] * 5 + case["W"])
    shape = (case["planes"], case["H"], case["W"])
    return torch.randint(0, 8, shape, generator=g).to(F32), torch.randint(0, 8, shape, generator=g).to(F32)


EXACT_C = (0.0625, 0.5)     # c1, c2 of the exact cases: dyadic, of the size (k dr)^2 takes for dr = 7 .. 25
EXACT_SHIFTS = ((0.0, 0.0), (3.0, 2.0))


def run_ssim_exact(ep: LibEntry, case, dev) -> None:
    p, t = integer_images(case)
    wy, wx = dyadic_taps(case["Ky"]), dyadic_taps(case["Kx"], phase=1)
    P, T = Poisoned(p, case, dev), Poisoned(t, case, dev)
    oh, ow = case["H"] - case["Ky"] + 1, case["W"] - case["Kx"] + 1
    maps = []
    for shift in EXACT_SHIFTS:
        want, bound = ssim_valid64(p, t, wy, wx, *EXACT_C, with_bound=True, sp=shift[0], st=shift[1])
        sums, fmap = ep.ssim(P, T, case, wy, wx, EXACT_C, shift, dev)
        err = (fmap.to(F64) - want).abs()
        ratio = float((err / bound).max())
        assert ratio <= 1.0, (case["name"], shift, ratio, float(err.max()))
        _note("ssim_window map (exact means)", ratio)
        own = torch.tensor([math.fsum(fmap[i].to(F64).flatten().tolist()) for i in range(case["planes"])], dtype=F64)
        fold = ssim_fold_depth(oh, ow) * U64 * fmap.to(F64).abs().sum((1, 2))
        assert bool(((sums - own).abs() <= fold).all()), (case["name"], shift, sums, own, fold)
        _note("ssim_window plane sums", float(((sums - own).abs() / fold).max()))
        no_map, _ = ep.ssim(P, T, case, wy, wx, EXACT_C, shift, dev, full=False)
        assert torch.equal(no_map, sums), (case["name"], "the sums depend on the map argument")
        maps.append((fmap.to(F64), bound))
    # the same images under two integer shifts: both within their bounds of one value
    (m0, b0), (m1, b1) = maps
    assert bool(((m0 - m1).abs() <= b0 + b1).all()), (case["name"], "the two shifts disagree")


def run_ssim_identical(ep: LibEntry, case, dev) -> None:
    """P == T: numerator and denominator are the same two fp32 factors -> 1.0 exactly, and the sums count the windows"""
    p, _ = integer_images(case)
    wy, wx = dyadic_taps(case["Ky"]), dyadic_taps(case["Kx"], phase=1)
    P = Poisoned(p, case, dev)
    oh, ow = case["H"] - case["Ky"] + 1, case["W"] - case["Kx"] + 1
    for shift in ((0.0, 0.0), (3.0, 3.0)):
        sums, fmap = ep.ssim(P, P, case, wy, wx, (1e-4, 9e-4), shift, dev)
        assert bool((fmap == 1.0).all()), (case["name"], shift, float((fmap - 1).abs().max()))
        assert bool((sums == float(oh * ow)).all()), (case["name"], shift, sums)


def run_ssim_real(ep: LibEntry, case, dev) -> None:
    """the kernel's map error against float64 at every offset within twice the fp32 library statement's own error at offset 0"""
    fx = real_fixture(case)
    geo = {"name": case["name"], "planes": 1, "H": case["H"], "W": case["W"], "Ky": case["K"], "Kx": case["K"], "rs": case["W"],
           "ps": case["H"] * case["W"], "off": 0}
    print(f"{case['name']}: yardstick max {fx['yard_max']:.3e} mean {fx['yard_mean']:.3e}")
    worst = []
    for off, o in fx["offsets"].items():
        shift = (float(o["p"].to(F64).mean().to(F32)), float(o["t"].to(F64).mean().to(F32)))
        sums, fmap = ep.ssim(Poisoned(o["p"], geo, dev), Poisoned(o["t"], geo, dev), geo, fx["taps"], fx["taps"], o["c"], shift, dev)
        e_max = float((fmap.to(F64) - o["map64"]).abs().max())
        e_mean = abs(float(sums[0]) / o["map64"].numel() - float(o["map64"].mean()))
        print(f"{case['name']} offset {off:g}: map error {e_max:.3e} ({e_max / fx['yard_max']:.3f} of the yardstick), "
              f"mean error {e_mean:.3e} ({e_mean / fx['yard_mean']:.3f})")
        _note(f"ssim_window real map error / yardstick, offset {off:g}", e_max / fx["yard_max"])
        _note(f"ssim_window real mean error / yardstick, offset {off:g}", e_mean / fx["yard_mean"])
        worst.append((off, e_max, e_mean))
    for off, e_max, e_mean in worst:
        assert e_max <= 2 * fx["yard_max"], (case["name"], off, e_max, fx["yard_max"])
        assert e_mean <= 2 * fx["yard_mean"], (case["name"], off, e_mean, fx["yard_mean"])


def run_ssim_refusals(ep: LibEntry, dev) -> None:
    """even K, K > VSX_SSIM_MAX_K, a plane smaller than the window and null pointers: the error code, and nothing is launched"""
    case = _sc("refusals", 4, 4, 5)
    p, t = integer_images(case)
    P, T = Poisoned(p, case, dev), Poisoned(t, case, dev)
    H, W = case["H"], case["W"]
    taps = torch.tensor(dyadic_taps(L.SSIM_MAX_K + 2)).to(dev)
    cs = torch.tensor([0.1, 0.2, 0.0, 0.0], dtype=F32).to(dev)
    sums, fmap, ws = Guarded((1,), F64, dev), Guarded((H * W,), F32, dev), Guarded((64,), F64, dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(P=P.ptr(), T=T.ptr(), H=H, W=W, wy=taps.data_ptr(), Ky=5, wx=taps.data_ptr(), Kx=5, c=cs.data_ptr(), shift=cs[2:].data_ptr(),
                 sums=sums.t.data_ptr(), ws=ws.t.data_ptr())
        a.update(kw)
        return ep.lib.vsx_ssim_window(a["P"], P.ps, P.rs, a["T"], T.ps, T.rs, 1, a["H"], a["W"], a["wy"], a["Ky"], a["wx"], a["Kx"], a["c"],
                                      a["shift"], a["sums"], fmap.t.data_ptr(), a["ws"], 64 * 8, st)

    bad = [dict(Ky=4), dict(Kx=6), dict(Ky=L.SSIM_MAX_K + 2), dict(Kx=L.SSIM_MAX_K + 2), dict(Ky=1), dict(H=4), dict(W=3), dict(P=None),
           dict(T=None), dict(wy=None), dict(wx=None), dict(c=None), dict(shift=None), dict(sums=None), dict(ws=None)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert ep.err().startswith("vsx_ssim_window"), (kw, ep.err())
    assert ep.lib.vsx_ssim_window_ws_bytes(1, H, W, 4, 5) == 0 and ep.lib.vsx_ssim_window_ws_bytes(1, 4, W, 5, 5) == 0
    out = Guarded((NQ,), F64, dev)
    for kw in (dict(P=None), dict(T=None), dict(out=None), dict(ws=None), dict(H=0), dict(W=0)):
        a = dict(P=P.ptr(), T=T.ptr(), H=H, W=W, out=out.t.data_ptr(), ws=ws.t.data_ptr())
        a.update(kw)
        assert ep.lib.vsx_pair_sums(a["P"], P.ps, P.rs, a["T"], T.ps, T.rs, 1, a["H"], a["W"], a["out"], a["ws"], 64 * 8, st) != 0, kw
        assert ep.err().startswith("vsx_pair_sums"), (kw, ep.err())
    assert ep.lib.vsx_pair_sums(P.ptr(), P.ps, P.rs, T.ptr(), T.ps, T.rs, 1, H, W, out.t.data_ptr(), ws.t.data_ptr(), 8, st) != 0  # short workspace
    torch.cuda.synchronize()
    assert sums.untouched() and fmap.untouched() and ws.untouched() and out.untouched(), "a refused call wrote an output"
    assert call() == 0, ep.err()  # the same arguments without the defect are served
    torch.cuda.synchronize()
    sums.check("refusals: served call")


# ------------------------------------------------------------------------------------------------ golden cases (reference's ssim_25d / ms_ssim_25d)
GOLDEN_FILE = "test_metrics.pt"
GOLDEN_CASES = {
    "d1_176": {"shape": (2, 1, 1, 176, 176), "seed": 21},
    "d5_176": {"shape": (1, 2, 5, 176, 176), "seed": 22},
    "anti_d1_176": {"shape": (2, 1, 1, 176, 176), "seed": 23, "anti": True},
}
GOLDEN_BETAS3 = (0.2, 0.3, 0.5)
GOLDEN_RTOL = 1e-3  # what tests/test_gpu_model.py::test_mixed_loss_vs_reference_golden allows the loss that carries the MS-SSIM term


def golden_stacks(name: str) -> tuple[torch.Tensor, torch.Tensor]:
    """target uniform, pred = target + 0.1 N(0, 1): correlated stacks, so the contrast term is positive at every scale and
    clamp=False raises no negative number to a fractional power.  ``anti``: pred = 1 - target + noise, the contrast term is negative at
    every scale and the clamp at 1e-4 decides the value (without it the result is NaN)"""
    c = GOLDEN_CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    target = torch.rand(c["shape"], generator=g)
    if c.get("anti"):
        return 1.0 - target + 0.1 * torch.randn(c["shape"], generator=g), target
    return target + 0.1 * torch.randn(c["shape"], generator=g), target


def golden_calls(name: str):
    """(key, function name, keywords) of every stored result of a case"""
    calls = [("ssim", "ssim_25d", dict(return_contrast_sensitivity=True)),
             ("ms_ssim_clamp", "ms_ssim_25d", dict(clamp=True)),
             ("ms_ssim_clamp_betas3", "ms_ssim_25d", dict(clamp=True, betas=GOLDEN_BETAS3))]
    if not GOLDEN_CASES[name].get("anti"):
        calls += [("ms_ssim", "ms_ssim_25d", dict(clamp=False)), ("ms_ssim_betas3", "ms_ssim_25d", dict(clamp=False, betas=GOLDEN_BETAS3))]
    return calls
