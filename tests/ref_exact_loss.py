"""Exact-arithmetic fixtures for the MixedLoss kernels of csrc/loss.hip at the level of their entry points: vsx_loss_pool,
vsx_loss_tmax, vsx_ssim_scale_fwd, vsx_ssim_scale_fwd_dmu, vsx_ssim_scale_fwd_fused, vsx_ssim_scale_bwd_in, vsx_loss_finalize.

The method is that of tests/ref_exact_head.py / tests/ref_exact_gemm.py: operands for which fp32 arithmetic is exact in any
order, so a statement is independent of tiling, atomics and summation order.

Dyadic stacks.  P and T hold k / 16, k in 0 .. 16 (the loss's operating range).  p, t, p p, t t, p t are multiples of 1/256 with
numerators of at most 8 bits: round_bf16 is the identity on them (asserted), every depth sum and 11 x 11 window sum is a multiple
of 1/256 below 2^24 / 256 (asserted) and exact in fp32 in any order.  A window mean is bf16(fp32(kb a)), kb = bf16(1 / (121 D)):
one correctly rounded product and one round-to-nearest-even, which torch on the CPU reproduces bit for bit.  The data range and
c1 = (0.01f dr)^2, c2 = (0.03f dr)^2 are plain fp32 products.  The pooled stacks of such a stack hold multiples of 1/64; their
products are rounded by bf16 (reproduced the same way) to multiples of 2^-12, whose window sums stay below 2^24 / 4096: the
second scale of the hand-made two-scale chain is stated in the same way.

torch.equal: Po / To, data ranges (max over the 64 slots), L1 / L2 sums (float64 sum over the slots), the slots vsx_loss_tmax
writes, the isolating backward cases, the sums of the P == T forward (every cs and ssim value is exactly 1 there: products of
two bf16 means are exact in fp32, so sx = sy = sxy and num = den bit for bit whether or not a b + c is contracted).

Derived bounds.  From bit-identical means the pixel formula (ssim_pixel) is a dozen fp32 operations.  ``RE`` evaluates it in
float64 together with a running error bound: a value v, a magnitude A >= |v| and the count k of rounded operations on the
longest path, such that |fl(v) - v| <= k u A to first order, u = 2^-24:
    x +- y   A = A_x + A_y (the sum of magnitudes)                              k = max(k_x, k_y) + 1
    x y      A = max(|v|, [k_x > 0] |y| A_x + [k_y > 0] |x| A_y)                k = max(k_x, k_y) + 1
    x / y    A = max(|v|, ([k_x > 0] A_x + [k_y > 0] |v| A_y) / |y|)            k = max(k_x, k_y) + 1
    a product with a constant that is 0 or a power of two, and a sum with an exact 0, are exact (k unchanged).
(err(x y) <= |y| k_x u A_x + |x| k_y u A_y + u |x y| and the like for the quotient; division and the bf16 means are correctly
rounded, contraction only removes roundings.)  K is the k of the output, counted from the source of ssim_pixel and pinned in
``K_PIXEL``; nothing else sets it.  The per-sample sums get (n + K) u sum |v|, n the terms per sample (atomics and block sums
give any order).  The combined backward case gets 6 u sum |terms| (2 p G and t G are exact, only the additions round).
vsx_loss_finalize gets a bound from the count of its products and powf calls (``finalize_statement``).

The float64 statements are written from oracle/loss_ref.py (metrics.py:272-349, mixed_loss.py:56-69 of the reference) with
unfold / avg_pool and share no code with the kernels' tiling.  ``TorchEntry`` is a plain-PyTorch fp32 implementation of the
seven entry points (box sums by convolution with ones); ``LibEntry`` wraps the library's.  The runners take either, so the same
tables run on the GPU and on the CPU.  ``DEFECTS`` are single indexing errors seeded into TorchEntry.  No GPU is needed to
import this module."""

from __future__ import annotations

import json
import os

import torch
import torch.nn.functional as F
from torch import Tensor

from tests.ref_exact_fnet3d import LIMIT, SLACK, U32, ints
from tests.ref_exact_gemm import Flags, _seed  # noqa: F401  (Flags is used by the GPU file)

F32, F64 = torch.float32, torch.float64
ST, SI = 32, 42                 # output tile and input footprint of the SSIM kernels
SLOTS, STRIDE = 64, 32          # VSX_LOSS_SLOTS, VSX_LOSS_SLOT_STRIDE
NAN, NINF = float("nan"), float("-inf")
BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
POW_ULP = 16                    # powf: OCML states OpenCL conformance, whose bound for pow is 16 ulp
FIELDS = ("dmx", "dmxx", "dmxy")
# rounded operations on the longest path of ssim_pixel (loss.hip), by output and by `last`; derived by RE, pinned here
K_PIXEL = {0: dict(cs=5, ssim=6, dmx=8, dmxx=6, dmxy=5), 1: dict(cs=5, ssim=6, dmx=10, dmxx=7, dmxy=5)}
K_COMBINED = 6


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def bf16r(x: Tensor) -> Tensor:
    """round_bf16 of an fp32 tensor (round to nearest even), as fp32"""
    assert x.dtype == F32
    return x.bfloat16().float()


def kb_of(D: int) -> Tensor:
    kb = bf16r(torch.tensor(1.0, dtype=F32) / torch.tensor(float(121 * D), dtype=F32))
    assert float(kb) == float(bf16r(torch.tensor(1.0 / (121 * D), dtype=F32)))   # no bf16 tie near 1 / (121 D)
    return kb


def f32v(x: float) -> float:
    """the value a C float argument or constant holds"""
    return float(torch.tensor(x, dtype=F32))


def record(tag: str, **kv) -> None:
    """measured ratios, appended as JSON lines to $VSX_RECORD (when set)"""
    path = os.environ.get("VSX_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": tag, **kv}) + "\n")


# ------------------------------------------------------------------------------------------------ dispatch arithmetic
def tile_plan(B: int, C: int, H: int, W: int, offset: int = 0) -> dict:
    """grids of the SSIM kernels: the forward covers the (H - 10) x (W - 10) outputs, the backward the H x W inputs, both in
    32 x 32 tiles x B C planes; xcd_tile() remaps a grid whose workgroup count is a multiple of 8; the one-pass forward takes
    8-byte loads (VEC) for an even W and 8-byte aligned stacks"""
    Ho, Wo = H - 10, W - 10
    fty, ftx, bty, btx = cdiv(Ho, ST), cdiv(Wo, ST), cdiv(H, ST), cdiv(W, ST)
    return dict(fwd=(fty, ftx), bwd=(bty, btx), fwd_total=fty * ftx * B * C, bwd_total=bty * btx * B * C,
                last_out=(Ho - ST * (fty - 1), Wo - ST * (ftx - 1)), last_own=(H - ST * (fty - 1), W - ST * (ftx - 1)),
                vec=W % 2 == 0 and offset % 2 == 0, odd=(H % 2, W % 2))


def stack_cases():
    def case(name, B, C, D, H, W, why, offset=0, bwd=True):
        p = tile_plan(B, C, H, W, offset)
        leg = (f"{why}: forward {p['fwd'][0]} x {p['fwd'][1]} tiles x {B * C} planes = {p['fwd_total']} workgroups "
               f"(total % 8 = {p['fwd_total'] % 8}), last tile {p['last_out'][0]} x {p['last_out'][1]} outputs owning "
               f"{p['last_own'][0]} x {p['last_own'][1]} inputs; backward {p['bwd'][0]} x {p['bwd'][1]} tiles = {p['bwd_total']} "
               f"workgroups (total % 8 = {p['bwd_total'] % 8}); {'VEC' if p['vec'] else 'non-VEC'}")
        return dict(name=name, B=B, C=C, D=D, H=H, W=W, offset=offset, bwd=bwd, leg=leg)
    return [
        case("one_pixel_1x3x1x11x11", 1, 3, 1, 11, 11, "one output pixel, D = 1, no XCD remap"),
        case("one_tile_1x1x5x42x42", 1, 1, 5, 42, 42, "exactly one full tile whose footprint ends on the image edge"),
        case("edge_2x2x5x43x43", 2, 2, 5, 43, 43, "a last tile of one output row / column that owns input rows / columns 32 .. 42, odd H and W, remap"),
        case("across_2x1x7x52x75", 2, 1, 7, 52, 75, "three tiles across, odd W, even H, D = 7"),
        case("vec_1x2x3x53x74", 1, 2, 3, 53, 74, "even W with 8-byte loads, odd H"),
        case("unaligned_1x2x3x53x74", 1, 2, 3, 53, 74, "the same stacks as views one float into a larger buffer: 4-byte alignment on an even W",
             offset=1, bwd=False),
        case("grids_1x2x3x65x33", 1, 2, 3, 65, 33, "the backward grid has 3 x 2 tiles where the forward has 2 x 1"),
        case("samples_3x2x2x64x64", 3, 2, 2, 64, 64, "B C = 6 planes of three samples, remap both ways"),
    ]


def chain_cases():
    byname = {c["name"]: c for c in stack_cases()}
    return [byname["edge_2x2x5x43x43"], byname["samples_3x2x2x64x64"]]


def pool_cases():
    return [dict(name="stride_8x515x515", planes=8, H=515, W=515, leg="8 x 258 x 258 = 532512 quads > 2048 x 256: the grid-stride loop runs twice, odd leftovers"),
            dict(name="tiny_3x7x5", planes=3, H=7, W=5, leg="36 quads in one workgroup, odd leftovers")]


TMAX_N = (1, 3, 5, 1023, 3 * 8192 + 5)
TMAX_WHERE = ("head", "tail", "last_wg", "negative")


def tmax_plan(n: int, head: int) -> dict:
    """vsx_loss_tmax: 16-byte loads from the first aligned element on, 8 per thread and launch; the elements before it and the
    tail go to workgroup 0; wave w of workgroup g writes slot (4 g + w) % 64"""
    h = min(head, n)
    n4 = (n - h) >> 2
    nblk = min(cdiv((n >> 2) + 1, 256 * 8), 4096)
    return dict(h=h, n4=n4, nblk=nblk, t0=h + 4 * n4)


def tmax_slot_of(n: int, head: int) -> Tensor:
    """the slot every element's value ends in"""
    p = tmax_plan(n, head)
    i = torch.arange(n)
    j = (i - p["h"]).div(4, rounding_mode="floor")
    body = (((j.div(256, rounding_mode="floor")) % p["nblk"]) * 4 + (j % 256).div(64, rounding_mode="floor")) % SLOTS
    edge_thread = torch.where(i < p["h"], i, i - p["t0"])
    return torch.where((i >= p["h"]) & (i < p["t0"]), body, edge_thread.div(64, rounding_mode="floor") % SLOTS)


# ------------------------------------------------------------------------------------------------ fixtures
_FIX: dict = {}


def clear_fixtures() -> None:
    _FIX.clear()


def dyadic(shape, seed: int, lo: int = 0, hi: int = 16, den: int = 16) -> Tensor:
    return ints(shape, lo, hi, seed) / den


def stack_fixture(case) -> dict:
    fx = _FIX.get(case["name"])
    if fx is None:
        shape = tuple(case[k] for k in "BCDHW")
        s0 = _seed(f"{shape}")   # the unaligned case shares the stacks of the aligned one
        fx = _FIX[case["name"]] = dict(P=dyadic(shape, s0 + 1), T=dyadic(shape, s0 + 2))
    return fx


def window_sums(X: Tensor) -> Tensor:
    """[B, C, D, H, W] -> [B, C, H - 10, W - 10]: the (D, 11, 11) window sums"""
    return X.sum(2).unfold(2, 11, 1).unfold(3, 11, 1).sum((-1, -2))


# ------------------------------------------------------------------------------------------------ running error evaluation
class RE:
    """value, magnitude and operation count of a quantity computed in fp32 (see the module docstring)"""
    __slots__ = ("v", "A", "k")

    def __init__(self, v, A=None, k: int = 0):
        self.v = torch.as_tensor(v, dtype=F64)
        self.A = self.v.abs() if A is None else A
        self.k = k

    def _zero(self) -> bool:
        return self.k == 0 and not bool(self.v.any())

    def _pow2(self) -> bool:
        m, _ = torch.frexp(self.v)
        return self.k == 0 and bool(((m.abs() == 0.5) | (m == 0)).all())

    def __neg__(self):
        return RE(-self.v, self.A, self.k)

    def __add__(self, o):
        if o._zero():
            return self
        if self._zero():
            return o
        return RE(self.v + o.v, self.A + o.A, max(self.k, o.k) + 1)

    def __sub__(self, o):
        return self + (-o)

    def __mul__(self, o):
        if self._zero() or o._zero():
            return RE(torch.zeros(torch.broadcast_shapes(self.v.shape, o.v.shape), dtype=F64))
        v = self.v * o.v
        if self._pow2() or o._pow2():
            return RE(v, self.A * o.A, max(self.k, o.k))
        A = (self.k > 0) * o.v.abs() * self.A + (o.k > 0) * self.v.abs() * o.A
        return RE(v, torch.maximum(v.abs(), A), max(self.k, o.k) + 1)

    def __truediv__(self, o):
        v = self.v / o.v
        A = ((self.k > 0) * self.A + (o.k > 0) * v.abs() * o.A) / o.v.abs()
        return RE(v, torch.maximum(v.abs(), A), max(self.k, o.k) + 1)


def ssim_fields(m, c1: float, c2: float, last: int) -> dict:
    """ssim_pixel of loss.hip, operation by operation, on the five means: the maps of compute_ssim_and_cs_bf16 (oracle/loss_ref.py)
    and the gradient of the map this scale contributes (ssim for the last scale, cs for the others) w.r.t. mu_x, mu_xx, mu_xy"""
    mx, my, mxx, myy, mxy = (RE(t) for t in m)
    two, c1, c2 = RE(2.0), RE(c1), RE(c2)
    gs, gc = RE(1.0 if last else 0.0), RE(0.0 if last else 1.0)
    sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    A, Bd = two * sxy + c2, sx + sy + c2
    cs = A / Bd
    num, den = two * mx * my + c1, mx * mx + my * my + c1
    L = num / den
    ssim = L * cs
    dcs, dL = gc + gs * L, gs * cs
    dsxy, dsx = dcs * two / Bd, (-dcs) * cs / Bd
    dmx = dsx * (RE(-2.0) * mx) + dsxy * (-my) + dL * (two * my / den - num * two * mx / (den * den))
    return dict(ssim=ssim, cs=cs, dmx=dmx, dmxx=dsx, dmxy=dsxy, Bd=Bd)


def forward_statement(P: Tensor, T: Tensor, q: int = 8) -> dict:
    """float64 statement of one scale on stacks whose five terms, rounded to bf16, are multiples of 2^-q"""
    B, C, D, H, W = P.shape
    p32, t32 = P.float(), T.float()
    assert torch.equal(p32.double(), P) and torch.equal(t32.double(), T)
    raw = (p32, t32, p32 * p32, t32 * t32, p32 * t32)
    terms = [bf16r(x) for x in raw]
    kb = kb_of(D)
    means, amax = [], 0.0
    for x in terms:
        a = window_sums(x.double())
        s = a * 2.0 ** q
        assert torch.equal(s, s.round()) and float(s.max()) < LIMIT, f"window sums are not multiples of 2^-{q} below 2^24 / 2^{q}"
        amax = max(amax, float(s.max()))
        means.append(bf16r(kb * a.float()).double())
    dr = t32.max()
    k1, k2 = torch.tensor(0.01, dtype=F32) * dr, torch.tensor(0.03, dtype=F32) * dr
    c1, c2 = float(k1 * k1), float(k2 * k2)
    st = dict(means=means, dr=float(dr), c1=c1, c2=c2, identity=all(torch.equal(a, b) for a, b in zip(raw, terms)), sum_max=amax,
              fields={last: ssim_fields(means, c1, c2, last) for last in (0, 1)},
              Po=F.avg_pool3d(P, (1, 2, 2)), To=F.avg_pool3d(T, (1, 2, 2)), l1=float((P - T).abs().sum()), l2=float(((P - T) ** 2).sum()),
              npix=C * (H - 10) * (W - 10))
    st["bd_min"] = float(st["fields"][0]["Bd"].v.min())
    return st


def case_statement(case, same: bool = False) -> dict:
    fx = stack_fixture(case)
    key = "st_same" if same else "st"
    if key not in fx:
        fx[key] = forward_statement(fx["T"] if same else fx["P"], fx["T"])
        assert fx[key]["identity"], case["name"] + ": round_bf16 is not the identity on the five terms"
        assert fx[key]["l2"] * 256 < LIMIT and fx[key]["l1"] * 16 < LIMIT
    return fx[key]


# ------------------------------------------------------------------------------------------------ buffers
def place(t: Tensor, dev, offset: int = 0) -> Tensor:
    """fp32 copy on ``dev``, as a view ``offset`` floats into a larger buffer"""
    buf = torch.empty(t.numel() + offset, dtype=F32, device=dev)
    buf[offset:] = t.flatten().float().to(dev)
    v = buf[offset:].view(t.shape)
    assert (v.data_ptr() - buf.data_ptr()) == 4 * offset and buf.data_ptr() % 16 == 0
    return v


def nans(n, dev) -> Tensor:
    return torch.full((int(n),) if isinstance(n, int) else tuple(n), NAN, dtype=F32, device=dev)


def slotted(fill: float, dev, values=None) -> Tensor:
    """a slotted accumulator: SLOTS values STRIDE floats apart; the floats between them are NaN and stay NaN"""
    buf = nans(SLOTS * STRIDE, dev)
    buf[::STRIDE] = fill
    if values is not None:
        buf[::STRIDE] = values.float().to(dev)
    return buf


def slots_of(buf: Tensor) -> Tensor:
    b = buf.detach().cpu()
    gaps = b.view(SLOTS, STRIDE)[:, 1:]
    assert bool(gaps.isnan().all()), "a float between two slots was written"
    return b[::STRIDE].double()


def range_slots(dr: float, where: int, dev) -> Tensor:
    """the data range as a reader of the slotted form must find it: in slot ``where`` alone, smaller values and -inf elsewhere"""
    v = torch.full((SLOTS,), NINF, dtype=F64)
    v[(where + 7) % SLOTS], v[(where + 30) % SLOTS], v[where] = 0.5 * dr, -dr, dr
    return slotted(NINF, dev, v)


def assert_equal(got: Tensor, ref64: Tensor, what: str) -> None:
    g = got.detach().cpu().double().reshape(ref64.shape)
    if not torch.equal(g, ref64):
        bad = (g != ref64) | g.isnan()
        idx = bad.nonzero()[0].tolist() if bad.any() else []
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: got {g[tuple(idx)].item() if idx else None}, "
                             f"statement {ref64[tuple(idx)].item() if idx else None}")


def assert_within(got: Tensor, r: RE, K: int, what: str) -> float:
    """|got - v| <= K u A per element; returns the worst |got - v| / (u A)"""
    assert r.k == K, f"{what}: the statement counts {r.k} rounded operations, the table says {K}"
    g = got.detach().cpu().double().reshape(r.v.shape)
    err = (g - r.v).abs()
    ok = err <= K * U32 * r.A * SLACK
    ratio = float((err / (U32 * r.A).clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    if not bool(ok.all()):
        idx = (~ok).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements past {K} u A (worst {ratio:.3g} u A), first at {idx}: "
                             f"got {g[tuple(idx)].item()!r}, statement {r.v[tuple(idx)].item()!r}")
    return ratio


def assert_sums(got: Tensor, old: Tensor, r: RE, K: int, B: int, what: str) -> float:
    """per-sample sums: |got - (old + sum v)| <= (n + K) u (|old| + sum |v|), n the terms per sample"""
    v = r.v.reshape(B, -1)
    n = v.shape[1] + 1
    ref, mag = old + v.sum(1), old.abs() + v.abs().sum(1)
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / (U32 * mag)).nan_to_num(nan=float("inf")).max())
    assert bool((err <= (n + K) * U32 * mag * SLACK).all()), f"{what}: {ratio:.3g} u sum|v| > n + K = {n + K} (got {got.tolist()}, statement {ref.tolist()})"
    return ratio / (n + K)


# ------------------------------------------------------------------------------------------------ the entry points
class LibEntry:
    """the library's entry points, taking tensors: device pointers, the current stream and the return code are handled here"""

    def __init__(self, lib):
        from viscy_amd import _lib
        self._lib, self._mod = lib, _lib

    def __getattr__(self, name):
        if not name.startswith("vsx_"):
            raise AttributeError(name)
        fn = getattr(self._lib, name)

        def call(*args):
            a = [self._mod.ptr(x) if (x is None or isinstance(x, Tensor)) else x for x in args]
            self._mod.check(fn(*a, self._mod.stream()), name)
        return call


DEFECTS = ("l1_column_twice", "last_rows_unpooled", "coef_by_bc", "coef_slots_swapped", "slot_left_out", "dpnext_at_leftover")


class TorchEntry:
    """plain PyTorch (fp32, CPU) of the seven entry points, with the rounding points of loss.hip's header comment and none of its
    tiling: box sums are convolutions with ones.  A slotted accumulator gets plane bc's share in slot bc % 64.  ``defect``
    seeds one indexing error (DEFECTS)."""

    def __init__(self, defect: str | None = None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # -- helpers
    @staticmethod
    def _pool(x: Tensor) -> Tensor:
        Hn, Wn = x.shape[-2] // 2, x.shape[-1] // 2
        a = x[..., 0:2 * Hn:2, 0:2 * Wn:2] + x[..., 0:2 * Hn:2, 1:2 * Wn:2]
        return 0.25 * ((a + x[..., 1:2 * Hn:2, 0:2 * Wn:2]) + x[..., 1:2 * Hn:2, 1:2 * Wn:2])

    @staticmethod
    def _amax(acc: Tensor, i: int, v: Tensor) -> None:
        if float(v) > NINF:
            acc[i] = torch.maximum(acc[i], v)

    def _range(self, tmax: Tensor, slots: bool) -> Tensor:
        if not slots:
            return tmax[0]
        return tmax[::STRIDE][:SLOTS - 1 if self.defect == "slot_left_out" else SLOTS].max()

    @staticmethod
    def _means(P, T, B, C, D, H, W):
        p, t = P.reshape(B * C, D, H, W), T.reshape(B * C, D, H, W)
        kb, ones = kb_of(D), torch.ones(1, 1, 11, 11)
        return [bf16r(kb * F.conv2d(bf16r(x).sum(1)[:, None], ones)[:, 0]) for x in (p, t, p * p, t * t, p * t)]

    @staticmethod
    def _maps(m, dr, last, bwd):
        mx, my, mxx, myy, mxy = m
        k1, k2 = torch.tensor(0.01) * dr, torch.tensor(0.03) * dr
        c1, c2 = k1 * k1, k2 * k2
        sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
        Bd, den = sx + sy + c2, mx * mx + my * my + c1
        cs = (2 * sxy + c2) / Bd
        num = 2 * mx * my + c1
        L = num / den
        if not bwd:
            return L * cs, cs, None
        dcs, dL = (L, cs) if last else (torch.ones_like(cs), torch.zeros_like(cs))
        dsxy, dsx = 2 * dcs / Bd, -dcs * cs / Bd
        dmx = dsx * (-2 * mx) + dsxy * (-my) + dL * (2 * my / den - num * 2 * mx / (den * den))
        return L * cs, cs, torch.stack([dmx, dsx, dsxy])

    def _scale(self, P, T, dr, sum_ssim, sum_cs, dmu, B, C, D, H, W, last, bwd):
        ssim, cs, f = self._maps(self._means(P, T, B, C, D, H, W), dr, last, bwd)
        sum_ssim[:B] += ssim.reshape(B, -1).sum(1)
        sum_cs[:B] += cs.reshape(B, -1).sum(1)
        if bwd:
            dmu.view(-1)[:f.numel()] = f.reshape(-1)

    # -- entry points
    def vsx_loss_pool(self, P, T, Po, To, tmax, l1sum, l2sum, planes, H, W):
        p, t = P.reshape(planes, H, W), T.reshape(planes, H, W)
        if Po is not None:
            Po.view(-1)[:] = self._pool(p).reshape(-1)
            To.view(-1)[:] = self._pool(t).reshape(-1)
        self._amax(tmax, 0, t.max())
        if l1sum is not None:
            l1sum[0] += (p - t).abs().sum()
            l2sum[0] += ((p - t) ** 2).sum()

    def vsx_loss_tmax(self, T, n, tmax):
        t = T.reshape(-1)[:n]
        pl = tmax_plan(n, ((16 - (T.data_ptr() & 15)) & 15) >> 2)
        body = t[pl["h"]:pl["t0"]].view(-1, 4).amax(1) if pl["n4"] else t[:0]
        for g in range(pl["nblk"]):
            for w in range(4):
                parts = [body[r + 64 * w:r + 64 * (w + 1)] for r in range(256 * g, pl["n4"], 256 * pl["nblk"])]
                if g == 0:
                    parts += [t[64 * w:min(64 * (w + 1), pl["h"])], t[pl["t0"] + 64 * w:pl["t0"] + 64 * (w + 1)]]
                v = torch.cat(parts) if parts else t[:0]
                if v.numel():
                    self._amax(tmax, ((4 * g + w) % SLOTS) * STRIDE, v.max())

    def vsx_ssim_scale_fwd(self, P, T, tmax, sum_ssim, sum_cs, B, C, D, H, W):
        self._scale(P, T, self._range(tmax, False), sum_ssim, sum_cs, None, B, C, D, H, W, 0, False)

    def vsx_ssim_scale_fwd_dmu(self, P, T, tmax, sum_ssim, sum_cs, dmu, B, C, D, H, W, last):
        self._scale(P, T, self._range(tmax, False), sum_ssim, sum_cs, dmu, B, C, D, H, W, last, True)

    def vsx_ssim_scale_fwd_fused(self, P, T, tmax, sum_ssim, sum_cs, dmu, Po, To, tmax_next, l1sum, l2sum, B, C, D, H, W, last):
        self._scale(P, T, self._range(tmax, True), sum_ssim, sum_cs, dmu, B, C, D, H, W, last, True)
        p, t = P.reshape(B * C, D, H, W), T.reshape(B * C, D, H, W)
        if Po is not None:
            po, to = self._pool(p), self._pool(t)
            if self.defect == "last_rows_unpooled":   # the last tile pools the 32 rows at its origin only
                keep = 16 * cdiv(H - 10, ST)
                Po.view(B * C, D, H // 2, W // 2)[:, :, :keep] = po[:, :, :keep]
                To.view(B * C, D, H // 2, W // 2)[:, :, :keep] = to[:, :, :keep]
                to = to[:, :, :keep]
            else:
                Po.view(-1)[:] = po.reshape(-1)
                To.view(-1)[:] = to.reshape(-1)
            for bc in range(B * C):
                self._amax(tmax_next, (bc % SLOTS) * STRIDE, to[bc].max())
        if l1sum is not None:
            d = p - t
            for bc in range(B * C):
                s = (bc % SLOTS) * STRIDE
                l1sum[s] += d[bc].abs().sum()
                l2sum[s] += (d[bc] ** 2).sum()
                if self.defect == "l1_column_twice" and W > ST:   # the first tile row counts footprint column 32 as well
                    l1sum[s] += d[bc][:, :ST, ST].abs().sum()

    def vsx_ssim_scale_bwd_in(self, P, T, dmu, coef, dPnext, dP, B, C, D, H, W, l1c, l2c, gout, has_ssim, last):
        p, t = P.reshape(B, C, D, H, W), T.reshape(B, C, D, H, W)
        g = torch.zeros_like(p)
        if has_ssim:
            Ho, Wo = H - 10, W - 10
            idx = torch.arange(B * C)
            idx = idx % B if self.defect == "coef_by_bc" else idx // C
            slot = (0 if last else 1) ^ (self.defect == "coef_slots_swapped")
            gs = coef.view(-1)[2 * idx + slot]
            S = bf16r(dmu.view(3, B * C, Ho, Wo) * gs[None, :, None, None])
            G = bf16r(kb_of(D) * F.conv2d(F.pad(S.view(-1, 1, Ho, Wo), (10, 10, 10, 10)), torch.ones(1, 1, 11, 11)))
            G = G.view(3, B, C, 1, H, W)
            g = G[0] + 2.0 * p * G[1] + t * G[2]
        if dPnext is not None:
            n = dPnext.view(B, C, D, H // 2, W // 2)
            if self.defect == "dpnext_at_leftover":
                iy, ix = (torch.arange(H) // 2).clamp_max(H // 2 - 1), (torch.arange(W) // 2).clamp_max(W // 2 - 1)
                up = n[..., iy, :][..., ix]
            else:
                up = F.pad(n.repeat_interleave(2, -2).repeat_interleave(2, -1), (0, W % 2, 0, H % 2))
            g = g + 0.25 * up
        gsc = gout[0] if gout is not None else torch.tensor(1.0)
        d = p - t
        if l1c != 0.0:
            g = g + torch.tensor(l1c) * gsc * torch.sign(d)
        if l2c != 0.0:
            g = g + 2.0 * (torch.tensor(l2c) * gsc) * d
        dP.view(-1)[:] = g.expand(B, C, D, H, W).reshape(-1)

    def vsx_loss_finalize(self, sum_ssim, sum_cs, l1sum, l2sum, npix, nelem, B, nscale, sum_slots, a1, a2, a3, gout, loss, coef, ms_out):
        a1, a2, a3, nelem = (torch.tensor(x, dtype=F32) for x in (a1, a2, a3, nelem))
        go = gout[0] if gout is not None else torch.tensor(1.0)
        ms = torch.tensor(0.0)
        if float(a3) != 0.0:
            betas = torch.tensor(BETAS, dtype=F32)[:nscale]
            raw = torch.stack([(sum_ssim if s == nscale - 1 else sum_cs)[s * B:(s + 1) * B] / npix[s] for s in range(nscale)])
            clamped = raw < torch.tensor(1e-4)
            v = torch.where(clamped, torch.tensor(1e-4), raw)
            prod = (v ** betas[:, None]).prod(0)
            g = -a3 * go / float(B) * betas[:, None] * prod[None] / v / npix[:nscale, None]
            g = torch.where(clamped, torch.zeros_like(g), g)
            c = torch.zeros(nscale, B, 2)
            c[:-1, :, 1] = g[:-1]
            c[-1, :, 0] = g[-1]
            coef.view(-1)[:c.numel()] = c.reshape(-1)
            ms = prod.sum() / float(B)
        n = max(sum_slots, 1)
        l = torch.tensor(0.0)
        if float(a1) != 0.0:
            l = l + a1 * l1sum[:n * STRIDE:STRIDE].sum() / nelem
        if float(a2) != 0.0:
            l = l + a2 * l2sum[:n * STRIDE:STRIDE].sum() / nelem
        if float(a3) != 0.0:
            l = l + a3 * (1.0 - ms)
        loss[0] = l
        if ms_out is not None:
            ms_out[0] = ms


# ------------------------------------------------------------------------------------------------ runners: forward of one scale
def _check_scale(tag, what, st, last, sums, olds, dmu, B, bwd=True) -> None:
    """the sums and (``bwd``) the three fields of one forward launch against the statement"""
    f, K = st["fields"][last], K_PIXEL[last]
    rs = assert_sums(sums[0], olds[0], f["ssim"], K["ssim"], B, what + " sum_ssim")
    rc = assert_sums(sums[1], olds[1], f["cs"], K["cs"], B, what + " sum_cs")
    rec = dict(sum_ssim=rs, sum_cs=rc)
    if bwd:
        d = dmu.detach().cpu().view(3, *f["dmx"].v.shape)
        for i, name in enumerate(FIELDS):
            rec[name] = assert_within(d[i], f[name], K[name], f"{what} {name} (last = {last})") / K[name]
    record(tag, **rec)


def _olds(B, seed, dev):
    o = [ints((B,), 1, 9, seed), ints((B,), 1, 9, seed + 1)]
    return o, [x.float().to(dev) for x in o]


def run_forward_case(ep, case, dev) -> None:
    """the three forward entry points on the same stacks against the same statement; the pooling pass and the one-pass kernel's
    pooling against the same Po / To / range / L1 / L2; the P == T stacks"""
    B, C, D, H, W = (case[k] for k in "BCDHW")
    fx, st, name = stack_fixture(case), case_statement(case), case["name"]
    P, T = place(fx["P"], dev, case["offset"]), place(fx["T"], dev, case["offset"])
    s0, nd = _seed(name), 3 * B * C * (H - 10) * (W - 10)
    total = tile_plan(B, C, H, W)["fwd_total"]
    dr1 = torch.tensor([st["dr"]], dtype=F32, device=dev)
    # vsx_ssim_scale_fwd
    olds, sums = _olds(B, s0, dev)
    ep.vsx_ssim_scale_fwd(P, T, dr1, sums[0], sums[1], B, C, D, H, W)
    _check_scale(f"{name}/fwd", f"ssim_scale_fwd {name}", st, 0, sums, olds, None, B, bwd=False)
    # vsx_ssim_scale_fwd_dmu
    for last in (0, 1):
        olds, sums = _olds(B, s0 + 2 + last, dev)
        dmu = nans(nd, dev)
        ep.vsx_ssim_scale_fwd_dmu(P, T, dr1, sums[0], sums[1], dmu, B, C, D, H, W, last)
        _check_scale(f"{name}/fwd_dmu/last{last}", f"ssim_scale_fwd_dmu {name}", st, last, sums, olds, dmu, B)
    # vsx_loss_pool: this scale's range, pooled stacks, L1 / L2; then the pooled target's range
    Po, To = nans(st["Po"].shape, dev), nans(st["To"].shape, dev)
    tm, l12 = torch.full((1,), NINF, dtype=F32, device=dev), torch.tensor([3.0, 5.0], dtype=F32, device=dev)
    ep.vsx_loss_pool(P, T, Po, To, tm, l12[0:1], l12[1:2], B * C * D, H, W)
    assert_equal(Po, st["Po"], f"loss_pool {name} Po")
    assert_equal(To, st["To"], f"loss_pool {name} To")
    assert_equal(tm, torch.tensor([st["dr"]], dtype=F64), f"loss_pool {name} range")
    assert_equal(l12, torch.tensor([3.0 + st["l1"], 5.0 + st["l2"]], dtype=F64), f"loss_pool {name} L1 / L2 sums (+ old 3, 5)")
    tm = torch.full((1,), NINF, dtype=F32, device=dev)
    ep.vsx_loss_pool(Po, To, None, None, tm, None, None, B * C * D, H // 2, W // 2)
    dr_next = float(st["To"].max())
    assert_equal(tm, torch.tensor([dr_next], dtype=F64), f"loss_pool {name} range of the pooled target, no outputs")
    # vsx_ssim_scale_fwd_fused: with and without the pooled outputs, with and without the L1 / L2 sums
    for i, (last, with_l1) in enumerate([(0, True), (0, False), (1, True), (1, False)]):
        what = f"ssim_scale_fwd_fused {name} last = {last}, L1 / L2 {'on' if with_l1 else 'off'}"
        olds, sums = _olds(B, s0 + 4 + i, dev)
        dmu = nans(nd, dev)
        tmax = range_slots(st["dr"], (s0 + 21 * i) % SLOTS if i else SLOTS - 1, dev)
        Po, To, tnext = (None, None, None) if last else (nans(st["Po"].shape, dev), nans(st["To"].shape, dev), slotted(NINF, dev))
        old1, old2 = ints((SLOTS,), 0, 3, s0 + 9), ints((SLOTS,), 0, 3, s0 + 10)
        l1, l2 = (slotted(0.0, dev, old1), slotted(0.0, dev, old2)) if with_l1 else (None, None)
        ep.vsx_ssim_scale_fwd_fused(P, T, tmax, sums[0], sums[1], dmu, Po, To, tnext, l1, l2, B, C, D, H, W, last)
        _check_scale(f"{name}/fwd_fused/last{last}", what, st, last, sums, olds, dmu, B)
        if not last:
            assert_equal(Po, st["Po"], what + " Po")
            assert_equal(To, st["To"], what + " To")
            sl = slots_of(tnext)
            assert float(sl.max()) == dr_next, f"{what}: range of the pooled target {float(sl.max())!r}, statement {dr_next!r}"
            assert bool((sl[total:] == NINF).all()), what + ": a range slot beyond the workgroup count was written"
        if with_l1:
            s1, s2 = slots_of(l1), slots_of(l2)
            assert float(s1.sum()) == float(old1.sum()) + st["l1"], f"{what}: L1 sum over the slots {float(s1.sum())!r}, statement {float(old1.sum()) + st['l1']!r}"
            assert float(s2.sum()) == float(old2.sum()) + st["l2"], f"{what}: L2 sum over the slots {float(s2.sum())!r}, statement {float(old2.sum()) + st['l2']!r}"
            assert torch.equal(s1[total:], old1[total:]) and torch.equal(s2[total:], old2[total:]), what + ": a sum slot beyond the workgroup count changed"
    # P == T: every cs and ssim value is exactly 1, so the sums count every output pixel of every tile exactly once
    same = case_statement(case, same=True)
    assert same["npix"] == C * (H - 10) * (W - 10)
    want = lambda o: torch.stack(o) + float(same["npix"])
    olds, sums = _olds(B, s0 + 11, dev)
    ep.vsx_ssim_scale_fwd(T, T, dr1, sums[0], sums[1], B, C, D, H, W)
    assert_equal(torch.stack(sums), want(olds), f"ssim_scale_fwd {name} P == T: old + C (H - 10) (W - 10)")
    for last in (0, 1):
        olds, sums = _olds(B, s0 + 12 + last, dev)
        dmu = nans(nd, dev)
        ep.vsx_ssim_scale_fwd_dmu(T, T, dr1, sums[0], sums[1], dmu, B, C, D, H, W, last)
        assert_equal(torch.stack(sums), want(olds), f"ssim_scale_fwd_dmu {name} P == T, last = {last}")
        olds, sums = _olds(B, s0 + 14 + last, dev)
        dmu2 = nans(nd, dev)
        ep.vsx_ssim_scale_fwd_fused(T, T, range_slots(st["dr"], 5, dev), sums[0], sums[1], dmu2, None, None, None, None, None, B, C, D, H, W, last)
        assert_equal(torch.stack(sums), want(olds), f"ssim_scale_fwd_fused {name} P == T, last = {last}")
        f, K = same["fields"][last], K_PIXEL[last]
        for dm, which in ((dmu, "fwd_dmu"), (dmu2, "fwd_fused")):
            for j, fname in enumerate(FIELDS):
                assert_within(dm.cpu().view(3, *f["dmx"].v.shape)[j], f[fname], K[fname], f"ssim_scale_{which} {name} P == T {fname} (last = {last})")


def run_chain_case(ep, case, dev) -> None:
    """two scales by hand: scale 0 through the one-pass kernel, then scale 1 on the Po, To and slotted range it produced"""
    B, C, D, H, W = (case[k] for k in "BCDHW")
    fx, st0, name = stack_fixture(case), case_statement(case), case["name"]
    if "st1" not in fx:
        fx["st1"] = forward_statement(st0["Po"], st0["To"], q=12)
    st1 = fx["st1"]
    H1, W1 = H // 2, W // 2
    assert H1 >= 11 and W1 >= 11 and not st1["identity"]   # the pooled products are really rounded by bf16 here
    P, T = place(fx["P"], dev), place(fx["T"], dev)
    s0 = _seed(name) + 40
    t0 = slotted(NINF, dev)
    ep.vsx_loss_tmax(T, T.numel(), t0)
    assert float(slots_of(t0).max()) == st0["dr"]
    olds0, sums0 = _olds(B, s0, dev)
    olds1, sums1 = _olds(B, s0 + 2, dev)
    dmu0, dmu1 = nans(3 * st0["npix"] * B, dev), nans(3 * st1["npix"] * B, dev)
    Po, To, t1 = nans(st0["Po"].shape, dev), nans(st0["To"].shape, dev), slotted(NINF, dev)
    l1, l2 = slotted(0.0, dev), slotted(0.0, dev)
    ep.vsx_ssim_scale_fwd_fused(P, T, t0, sums0[0], sums0[1], dmu0, Po, To, t1, l1, l2, B, C, D, H, W, 0)
    ep.vsx_ssim_scale_fwd_fused(Po, To, t1, sums1[0], sums1[1], dmu1, None, None, None, None, None, B, C, D, H1, W1, 1)
    _check_scale(f"{name}/chain/scale0", f"chain {name} scale 0", st0, 0, sums0, olds0, dmu0, B)
    assert_equal(Po, st0["Po"], f"chain {name} Po")
    assert_equal(To, st0["To"], f"chain {name} To")
    assert float(slots_of(t1).max()) == st1["dr"], f"chain {name}: the range scale 1 reads"
    assert float(slots_of(l1).sum()) == st0["l1"] and float(slots_of(l2).sum()) == st0["l2"]
    _check_scale(f"{name}/chain/scale1", f"chain {name} scale 1 ({H1} x {W1})", st1, 1, sums1, olds1, dmu1, B)


# ------------------------------------------------------------------------------------------------ runners: pooling pass, stack maximum
def run_pool_case(ep, case, dev) -> None:
    planes, H, W, name = case["planes"], case["H"], case["W"], case["name"]
    s0 = _seed(name)
    P, T = dyadic((planes, H, W), s0 + 1, 0, 2, 2), dyadic((planes, H, W), s0 + 2, 0, 2, 2)
    l1, l2 = float((P - T).abs().sum()), float(((P - T) ** 2).sum())
    assert (l1 + 8) * 2 < LIMIT and (l2 + 8) * 4 < LIMIT, "L1 is a multiple of 1/2, L2 of 1/4: both sums must stay below 2^24 units"
    Pd, Td = place(P, dev), place(T, dev)
    Po, To = nans((planes, H // 2, W // 2), dev), nans((planes, H // 2, W // 2), dev)
    tm, l12 = torch.full((1,), NINF, dtype=F32, device=dev), torch.tensor([7.0, 2.0], dtype=F32, device=dev)
    ep.vsx_loss_pool(Pd, Td, Po, To, tm, l12[0:1], l12[1:2], planes, H, W)
    assert_equal(Po, F.avg_pool2d(P, 2), f"loss_pool {name} Po")
    assert_equal(To, F.avg_pool2d(T, 2), f"loss_pool {name} To")
    assert_equal(tm, T.max().reshape(1), f"loss_pool {name} range")
    assert_equal(l12, torch.tensor([7.0 + l1, 2.0 + l2], dtype=F64), f"loss_pool {name} L1 / L2 sums (+ old 7, 2)")
    # the maximum in the odd leftover row alone; no pooled outputs, no sums
    T2 = T.clone() * 0.5
    T2[planes - 1, H - 1, W // 3] = 1.0
    tm = torch.full((1,), NINF, dtype=F32, device=dev)
    ep.vsx_loss_pool(Pd, place(T2, dev), None, None, tm, None, None, planes, H, W)
    assert_equal(tm, torch.ones(1, dtype=F64), f"loss_pool {name} range from the leftover row")


def tmax_data(n: int, where: str, seed: int):
    """values and the index that holds the maximum"""
    neg = where == "negative"
    v = -1.0 - dyadic((n,), seed) if neg else 0.5 * dyadic((n,), seed)
    at = {"head": 0, "tail": n - 1, "last_wg": min(n - 1, 3 + 4 * 800), "negative": n // 2}[where]
    v[at] = -0.5 if neg else 1.0
    return v, at


def run_tmax_case(ep, n: int, dev) -> None:
    for off in range(4):
        for where in TMAX_WHERE:
            v, at = tmax_data(n, where, _seed(f"tmax{n}") + off)
            T = place(v, dev, off)
            head = (4 - off) % 4
            assert ((16 - (T.data_ptr() & 15)) & 15) >> 2 == head
            slot = tmax_slot_of(n, head)
            want = torch.full((SLOTS,), NINF, dtype=F64).scatter_reduce(0, slot, v, "amax")
            buf = slotted(NINF, dev)
            ep.vsx_loss_tmax(T, n, buf)
            got = slots_of(buf)
            what = f"loss_tmax n = {n}, {off} floats past 16-byte alignment, maximum at {at} ({where})"
            assert float(got.max()) == float(v.max()) == (-0.5 if where == "negative" else 1.0), what
            assert_equal(got, want, what + ": slot values ((4 workgroup + wave) % 64; -inf where no wave wrote)")


# ------------------------------------------------------------------------------------------------ runners: backward of one scale
def box_T(S: Tensor) -> Tensor:
    """transposed box filter: [N, Ho, Wo] -> [N, Ho + 10, Wo + 10], out(y, x) = sum of S over [y - 10, y] x [x - 10, x]"""
    return F.conv2d(F.pad(S[:, None], (10, 10, 10, 10)), torch.ones(1, 1, 11, 11, dtype=S.dtype))[:, 0]


def bwd_coef(B: int) -> Tensor:
    """powers of two that differ per sample and per slot: sample 0 = {1/2, 1/4}, sample 1 = {2, 1}, sample 2 = {8, 4}"""
    return torch.tensor([[2.0 ** (2 * b - 1), 2.0 ** (2 * b - 2)] for b in range(B)], dtype=F64)


def bwd_statement(P, T, dmu, coef, dPn, l1c, l2c, gout, has_ssim, last):
    """float64: the terms of dP and their magnitudes"""
    B, C, D, H, W = P.shape
    gs = 1.0 if gout is None else gout
    terms = []
    if has_ssim:
        Ho, Wo = H - 10, W - 10
        g = coef[:, 0 if last else 1].repeat_interleave(C)
        prod = dmu.view(3, B * C, Ho, Wo).float() * g.float()[None, :, None, None]
        S = bf16r(prod)
        a = box_T(S.double().view(-1, Ho, Wo))
        G = bf16r(kb_of(D) * a.float()).double().view(3, B, C, 1, H, W)
        terms += [G[0].expand(B, C, D, H, W), 2.0 * P * G[1], T * G[2]]
        exact = torch.equal(S, prod) and torch.equal(a.float().double(), a)
    else:
        exact = True
    if dPn is not None:
        terms.append(0.25 * F.pad(dPn.repeat_interleave(2, -2).repeat_interleave(2, -1), (0, W % 2, 0, H % 2)))
    if l1c:
        terms.append(l1c * gs * torch.sign(P - T))
    if l2c:
        terms.append(2.0 * l2c * gs * (P - T))
    return sum(terms), sum(t.abs() for t in terms), exact


BWD_KINDS = ("x", "xx", "xy", "next", "l1", "l2", "combined")


def run_backward_case(ep, case, dev) -> None:
    """vsx_ssim_scale_bwd_in from hand-made fields and factors: one term at a time (bit-equal), then all at once (6 u sum |terms|)"""
    B, C, D, H, W = (case[k] for k in "BCDHW")
    fx, name, s0 = stack_fixture(case), case["name"], _seed(case["name"]) + 80
    Ho, Wo, Hn, Wn = H - 10, W - 10, H // 2, W // 2
    shape = (B, C, D, H, W)
    full = ints((3, B * C, Ho, Wo), -2, 2, s0 + 1)
    nxt = ints((B, C, D, Hn, Wn), -4, 4, s0 + 2)
    coef, gout, l1c, l2c = bwd_coef(B), 2.0, 0.125, 0.0625
    const = lambda v: torch.full(shape, v, dtype=F64)
    worst = 0.0
    for kind in BWD_KINDS:
        for last in (0, 1):
            P, T, dmu, dPn, a1, a2, has = fx["P"], fx["T"], None, None, 0.0, 0.0, 0
            if kind in ("x", "xx", "xy"):
                q = ("x", "xx", "xy").index(kind)
                dmu = torch.zeros_like(full)
                dmu[q] = full[q]
                P, T, has = const(0.5 if kind == "xx" else 0.0), const(1.0 if kind == "xy" else 0.0), 1
            elif kind == "next":
                P, T, dPn = const(0.0), const(0.0), nxt
            elif kind == "l1":
                a1 = l1c
            elif kind == "l2":
                a2 = l2c
            else:
                dmu, dPn, a1, a2, has = full, nxt, l1c, l2c, 1
            ref, mag, exact = bwd_statement(P, T, dmu, coef, dPn, a1, a2, gout, has, last)
            assert exact, f"{name} {kind}: the factor product or a 121-term sum is not exact"
            dP = nans(shape, dev)
            ep.vsx_ssim_scale_bwd_in(place(P, dev), place(T, dev), None if dmu is None else place(dmu, dev),
                                     place(coef, dev) if has else None, None if dPn is None else place(dPn, dev), dP, B, C, D, H, W,
                                     a1, a2, torch.tensor([gout], dtype=F32, device=dev), has, last)
            what = f"ssim_scale_bwd_in {name} {kind} last = {last} ([B, C, D, H, W])"
            if kind != "combined":
                if kind == "next":
                    assert not bool(ref[..., 2 * Hn:, :].any()) and not bool(ref[..., :, 2 * Wn:].any())
                if kind == "l1":
                    assert bool((P == T).any()) and set(ref.unique().tolist()) == {-0.25, 0.0, 0.25}
                assert_equal(dP, ref, what)
            else:
                err = (dP.cpu().double() - ref).abs()
                ratio = float((err / (U32 * mag).clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
                assert bool((err <= K_COMBINED * U32 * mag * SLACK).all()), f"{what}: worst {ratio:.3g} u sum|terms| > {K_COMBINED}"
                worst = max(worst, ratio / K_COMBINED)
    record(f"{name}/bwd_in/combined", dP=worst)


# ------------------------------------------------------------------------------------------------ runners: finalisation
def finalize_cases():
    out = []
    for B, nscale, slots, with_gout, (a1, a2, a3) in [
            (1, 3, 1, False, (0.5, 0.0, 0.5)), (3, 1, 64, True, (0.5, 0.25, 0.5)), (300, 5, 64, True, (0.5, 0.0, 0.5)),
            (3, 5, 1, False, (0.3, 0.2, 0.5)), (300, 3, 1, True, (0.0, 0.0, 1.0)), (3, 5, 64, True, (1.0, 0.0, 0.0)),
            (1, 3, 1, False, (0.0, 1.0, 0.0))]:
        out.append(dict(name=f"B{B}_s{nscale}_slots{slots}_g{int(with_gout)}_a{a1}_{a2}_{a3}", B=B, nscale=nscale, slots=slots,
                        gout=0.75 if with_gout else None, a=(a1, a2, a3)))
    return out


def finalize_fixture(case) -> dict:
    B, ns, s0 = case["B"], case["nscale"], _seed(case["name"])
    g = torch.Generator().manual_seed(s0)
    npix = torch.tensor([float(2 * (176 // 2 ** s) ** 2) for s in range(5)], dtype=F32)
    mean = 0.2 + 0.79 * torch.rand((5, B), generator=g, dtype=F64)
    mean[0, 0] = 5e-5                  # below the clamp
    mean[ns - 1, B - 1] = -0.3         # negative
    sums = (mean * npix.double()[:, None]).float()
    other = torch.rand((5, B), generator=g).float()   # the sums the loss does not use (ssim of scales 0 .. n - 2, cs of the last)
    ssum, csum = other.clone(), sums.clone()
    ssum[ns - 1], csum[ns - 1] = sums[ns - 1], other[ns - 1]
    l1s, l2s = 1000.0 * torch.rand(SLOTS, generator=g).float(), 300.0 * torch.rand(SLOTS, generator=g).float()
    return dict(npix=npix, ssum=ssum, csum=csum, l1s=l1s, l2s=l2s, nelem=float(2 * 5 * 176 * 176 * B))


def finalize_statement(case, fx) -> dict:
    """float64 of loss_finalize_kernel with its fp32 constants, and the bounds in units of u = 2^-24.
    Per scale: raw = sum / npix (1 u), powf (POW_ULP ulp = 2 POW_ULP u, + beta < 1 times the 1 u of its argument), the product
    (1 u): K_prod = (2 POW_ULP + 2) nscale.  coef = -a3 gout / B beta prod / v / npix: 6 operations + the 1 u of v.
    ms = (sum of B positive products: 1 addition per thread, 6 in the wave, 3 over the waves) / B: K_prod + 11.
    loss: a slot sum is positive (at most 64 additions), a s / nelem 2 more; 1 - ms and a3 (1 - ms) one each; the 3 final
    additions at most u times the sum of the terms each."""
    B, ns, n = case["B"], case["nscale"], max(case["slots"], 1)
    a1, a2, a3 = (f32v(x) for x in case["a"])
    go = 1.0 if case["gout"] is None else f32v(case["gout"])
    npix, betas = fx["npix"].double(), torch.tensor(BETAS, dtype=F32).double()[:ns]
    out = dict(coef=None, ms=0.0)
    kprod = (2 * POW_ULP + 2) * ns
    if a3 != 0.0:
        raw = torch.stack([(fx["ssum"] if s == ns - 1 else fx["csum"])[s].double() / npix[s] for s in range(ns)])
        lo = f32v(1e-4)
        clamped = raw.float() < torch.tensor(1e-4, dtype=F32)
        assert bool(clamped[0, 0]) and bool(clamped[ns - 1, B - 1]) and int(clamped.sum()) == 2
        v = torch.where(clamped, torch.tensor(lo, dtype=F64), raw)
        prod = (v ** betas[:, None]).prod(0)
        g = torch.where(clamped, torch.zeros_like(v), -a3 * go / B * betas[:, None] * prod[None] / v / npix[:ns, None])
        coef = torch.zeros(ns, B, 2, dtype=F64)
        coef[:-1, :, 1], coef[-1, :, 0] = g[:-1], g[-1]
        out.update(coef=coef, ms=float(prod.sum() / B), clamped=clamped, k_coef=kprod + 7)
    nelem = f32v(fx["nelem"])
    t1 = a1 * float(fx["l1s"][:n].double().sum()) / nelem if a1 != 0.0 else 0.0
    t2 = a2 * float(fx["l2s"][:n].double().sum()) / nelem if a2 != 0.0 else 0.0
    out["k_ms"] = kprod + 11
    out["loss"] = t1 + t2 + (a3 * (1.0 - out["ms"]) if a3 != 0.0 else 0.0)
    out["loss_bound"] = (SLOTS + 2 + 3) * (t1 + t2) + a3 * (out["k_ms"] * out["ms"] + (2 + 3) * abs(1.0 - out["ms"]))
    return out


def run_finalize_case(ep, case, dev) -> None:
    fx = finalize_fixture(case)
    st = finalize_statement(case, fx)
    B, ns, slots = case["B"], case["nscale"], case["slots"]
    what = f"loss_finalize {case['name']}"
    if slots > 1:
        l1, l2 = slotted(0.0, dev, fx["l1s"]), slotted(0.0, dev, fx["l2s"])
    else:
        l1, l2 = fx["l1s"][:1].to(dev), fx["l2s"][:1].to(dev)
    out, coef = nans(2, dev), nans(ns * B * 2, dev)
    gout = None if case["gout"] is None else torch.tensor([case["gout"]], dtype=F32, device=dev)
    ep.vsx_loss_finalize(fx["ssum"].reshape(-1).to(dev), fx["csum"].reshape(-1).to(dev), l1, l2, fx["npix"].to(dev), fx["nelem"], B, ns, slots,
                         *case["a"], gout, out[0:1], coef, out[1:2])
    got = out.cpu().double()
    eloss = abs(float(got[0]) - st["loss"]) / U32
    assert eloss <= st["loss_bound"] * SLACK, f"{what}: loss {float(got[0])!r}, statement {st['loss']!r}: {eloss:.3g} u > {st['loss_bound']:.3g} u"
    rec = dict(loss=eloss / st["loss_bound"])
    c = coef.cpu().double().view(ns, B, 2)
    if st["coef"] is None:
        assert float(got[1]) == 0.0 and bool(c.isnan().all()), what + ": a3 = 0 gives ms = 0 and leaves coef alone"
    else:
        ems = abs(float(got[1]) - st["ms"]) / (U32 * st["ms"])
        assert ems <= st["k_ms"] * SLACK, f"{what}: ms {float(got[1])!r}, statement {st['ms']!r}: {ems:.3g} u > {st['k_ms']} u"
        zero = st["coef"] == 0
        assert torch.equal(c[zero], torch.zeros_like(c[zero])), what + ": the unused slot of a scale and the factor of a clamped mean are exactly 0"
        ec = ((c - st["coef"]).abs() / (U32 * st["coef"].abs()).clamp_min(1e-300))[~zero]
        assert bool((ec <= st["k_coef"] * SLACK).all()), f"{what}: coef off by {float(ec.max()):.3g} u > {st['k_coef']} u"
        rec.update(ms=ems / st["k_ms"], coef=float(ec.max()) / st["k_coef"])
    record(f"finalize/{case['name']}", **rec)


# ------------------------------------------------------------------------------------------------ the whole loss through the entry points
def mixed_loss_via(ep, preds: Tensor, target: Tensor, a1: float, a2: float, a3: float, fused: bool = True, dev="cpu"):
    """MixedLossFn.forward / backward of viscy_amd/losses.py, restated on an object with the seven entry points: (loss, dP)"""
    B, C, D, H, W = preds.shape
    ns = 5
    w1 = SLOTS * STRIDE if fused else 4
    z = lambda n, v=0.0: torch.full((n,), v, dtype=F32, device=dev)
    l1sum, l2sum, tmax = z(w1), z(w1), [z(w1, NINF) for _ in range(ns)]
    sum_ssim, sum_cs = z(5 * B), z(5 * B)
    Ps, Ts, dims = [preds.float().to(dev)], [target.float().to(dev)], [(H, W)]
    for sc in range(ns - 1):
        h, w = dims[sc]
        Ps.append(nans((B, C, D, h // 2, w // 2), dev))
        Ts.append(nans((B, C, D, h // 2, w // 2), dev))
        dims.append((h // 2, w // 2))
    npix = torch.tensor([float(C * (h - 10) * (w - 10)) for h, w in dims], dtype=F32, device=dev)
    dmus = [nans(3 * B * C * (h - 10) * (w - 10), dev) for h, w in dims]
    sl = lambda t, sc: t[sc * B:(sc + 1) * B]
    if fused:
        ep.vsx_loss_tmax(Ts[0], Ts[0].numel(), tmax[0])
        for sc in range(ns):
            h, w = dims[sc]
            last = sc == ns - 1
            ep.vsx_ssim_scale_fwd_fused(Ps[sc], Ts[sc], tmax[sc], sl(sum_ssim, sc), sl(sum_cs, sc), dmus[sc], None if last else Ps[sc + 1],
                                        None if last else Ts[sc + 1], None if last else tmax[sc + 1], l1sum if sc == 0 else None,
                                        l2sum if sc == 0 else None, B, C, D, h, w, int(last))
    else:
        for sc in range(ns):
            h, w = dims[sc]
            last = sc == ns - 1
            ep.vsx_loss_pool(Ps[sc], Ts[sc], None if last else Ps[sc + 1], None if last else Ts[sc + 1], tmax[sc], l1sum if sc == 0 else None,
                             l2sum if sc == 0 else None, B * C * D, h, w)
        for sc in range(ns):
            h, w = dims[sc]
            ep.vsx_ssim_scale_fwd_dmu(Ps[sc], Ts[sc], tmax[sc], sl(sum_ssim, sc), sl(sum_cs, sc), dmus[sc], B, C, D, h, w, int(sc == ns - 1))
    out, coef = nans(2, dev), nans(ns * B * 2, dev)
    nelem = float(preds.numel())
    ep.vsx_loss_finalize(sum_ssim, sum_cs, l1sum, l2sum, npix, nelem, B, ns, SLOTS if fused else 1, a1, a2, a3, None, out[0:1], coef, out[1:2])
    dnext = None
    for sc in range(ns - 1, -1, -1):
        h, w = dims[sc]
        dP = nans((B, C, D, h, w), dev)
        ep.vsx_ssim_scale_bwd_in(Ps[sc], Ts[sc], dmus[sc], coef[sc * B * 2:(sc + 1) * B * 2], dnext, dP, B, C, D, h, w,
                                 a1 / nelem if sc == 0 else 0.0, a2 / nelem if sc == 0 else 0.0, None, 1, int(sc == ns - 1))
        dnext = dP
    return out[0].cpu(), dnext.cpu()
