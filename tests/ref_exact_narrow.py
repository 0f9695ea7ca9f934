"""Exact-arithmetic fixtures for the narrow-channel (VSCyto2D) kernels of csrc/narrow.hip at the level of their ten entry points:
vsx_narrow_stem_fwd / _stem_wgrad, vsx_narrow_proj_fwd / _proj_bwd, vsx_narrow_block_fwd1 / _fwd2 / _bwd_a / _bwd_b / _bwd_c and
vsx_narrow_voxel_shuffle_bwd.

The method is that of tests/ref_exact_loss.py / tests/ref_exact_gemm.py: operands for which fp32 arithmetic is exact in any order,
so a statement is independent of tiling, of the tiles a workgroup walks and of the order its partials are folded in.

Exact tier (torch.equal).  Operands are small integers; every fixture asserts that the sum of magnitudes of every reduction stays
below 2^24 and (bf16) that every stored value is a bf16 number.
  * stem forward / weight gradient, the shuffle adjoint (acc * inv is one fp32 product, restated in fp32 torch; for s = 3 it
    rounds, and the bf16 store rounds once more, both reproduced bit for bit), the depthwise output y of pass 1, pass C (dx, ddw, ddb),
    the projection's dxn / db;
  * projection with gamma = 0: xn == beta[k] whatever the LayerNorm produces, so out and dW = beta[k] sum_r d[r, c] are exact;
    mean = fl(S fl(1 / Ccat)) of an exact integer sum, restated in fp32 torch;
  * block passes with fc1 dead (W1f = 0) and GELU saturated (b1f[j] in {+-16, +-32}): h == b1f for every pixel, gelu_erf gives b1f[j]
    or 0, gelu_erf_grad gives 1 or 0 (exp(-128) underflows): the GRN sums n b1f^2, pass 2's out with integer per-sample s[b, :],
    pass A (dW2, db2, P, S) and pass B's db1f are exact, dy == 0 by value.  The assumption is that erff(+-11.3) is exactly +-1.
Stored outputs start as NaN between sentinel-filled guards; accumulated outputs (the += of the C-ABI) start from small integers
between the same guards.  After the call the guards are unchanged and no NaN is left.  ``LibEntry`` sizes the partials' scratch
from the Python restatement of blk_grid / stem_rows_per_wg / proj_wgs, asserts vsx_narrow_ws_floats says the same, hands the
kernels exactly that many NaN floats between guards and finds every one of them written: the dispatched grid is checked per case.

Bounded tier (float64 statement, per-element K u A).  Inputs are dyadic rationals that both dtypes hold exactly.  ``RE`` (of
ref_exact_loss) evaluates the kernels' formulas operation by operation in float64 with a running magnitude A and the count K of
rounded operations on the longest path; K per output is pinned in ``K_BLOCK`` / ``K_PROJ`` and nothing else sets it.  A library
function f enters through ``fn``: |err| <= |f'(x)| k_x u A_x + ulp(f) 2 u |f|, i.e. A = max(|f|, |f'| A_x), k = k_x + 2 ulp(f):
    ERF_ULP = 16    erff: the device library (OCML) states OpenCL conformance, whose bound for erf is 16 ulp
    RSQRT_ULP = 2   rsqrtf: OpenCL's bound for rsqrt is 2 ulp (the hardware instruction is documented at 1 ulp)
    EXP_K = 18      __expf(a) is the native path exp2(a log2(e)) on v_exp_f32.  In units of u relative to the result: the product
                    a log2(e) rounds once (u |a log2(e)| in the exponent, times ln 2 in the result: |a| <= 8 for |h| <= 4, where
                    a = -0.5 h h >= -8), the fp32 constant log2(e) is itself rounded (the same again: 8) and v_exp_f32 is documented
                    at 1 ulp (2 u): 8 + 8 + 2.  No accuracy statement for __expf itself is installed with the compiler, so this
                    constant is derived, not quoted.
A bf16 store adds U16 |v| (round to nearest even of 8 significant bits).  Sums over n terms get (n + K) u sum |v|.  The worst
observed ratios are recorded through ``record`` into profiles/narrow_exact_margins.txt.

``TorchEntry`` is a plain-PyTorch fp32 implementation of the ten entry points with the kernels' rounding points and none of their
tiling; ``LibEntry`` wraps the library's.  The runners take either, so the same tables run on the GPU and on the CPU.  ``DEFECTS``
are single indexing errors seeded into TorchEntry.  No GPU is needed to import this module."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import Tensor

from tests.ref_exact_fnet3d import LIMIT, SLACK, U16, U32, choice, ints
from tests.ref_exact_gemm import _seed
from tests.ref_exact_loss import RE, assert_equal, cdiv, record  # noqa: F401  (record is used by the test files as well)

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = {"fp32": F32, "bf16": BF16}
NAN, SENT, GUARD = float("nan"), 77.0, 64
NB, NWG_MAX, STEM_ROWS, STEM_EPT, PJ_V = 256, 2048, 64, 16, 12   # narrow.hip
OP_STEM, OP_PROJ, OP_FWD1, OP_BWD_A, OP_BWD_B, OP_BWD_C = range(6)   # VSX_NARROW_*
RSQRT2, RSQRT2PI = 0.70710678118654752, 0.3989422804014327      # the constants of gelu_erf / gelu_erf_grad
ERF_ULP, RSQRT_ULP, EXP_K = 16, 2, 18
EPS = 1e-6


def f32c(x: float) -> float:
    """the value a float constant of the kernel source holds"""
    return float(torch.tensor(x, dtype=F32))


# ------------------------------------------------------------------------------------------------ dispatch arithmetic
def blk_grid(B: int, hw: int) -> tuple[int, int]:
    """(workgroups per sample, tiles per workgroup) of the five per-pixel passes"""
    nt = cdiv(hw, NB)
    want = min(max(cdiv(NWG_MAX, B), 1), nt)
    tpw = cdiv(nt, want)
    return cdiv(nt, tpw), tpw


def stem_rows_per_wg(M0: int) -> int:
    return cdiv(cdiv(M0, 1024), STEM_ROWS) * STEM_ROWS


def proj_wgs(M: int) -> int:
    return min(cdiv(M, 16), 1024)


def ws_floats(op: int, B: int, n: int, C: int, K: int = 0) -> int:
    """vsx_narrow_ws_floats"""
    if op == OP_STEM:
        return cdiv(n, stem_rows_per_wg(n)) * (C * K + C)
    if op == OP_PROJ:
        return proj_wgs(n) * (C * K + C)
    G = B * blk_grid(B, n)[0]
    return G * {OP_FWD1: 4 * C, OP_BWD_A: C * 4 * C + C + 8 * C, OP_BWD_B: 4 * C * C + 4 * C, OP_BWD_C: 49 * C + C}[op]


def vec_elems(dt) -> int:
    return 4 if dt == F32 else 8


# ------------------------------------------------------------------------------------------------ buffers
class Guarded:
    """an output buffer between two sentinel-filled guards: NaN for a stored output, ``old`` for an accumulated one"""

    def __init__(self, shape, dtype, dev, old: Tensor | None = None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if old is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(old.to(dtype).reshape(shape))
        assert self.t.data_ptr() % 16 == 0

    def check(self, what: str) -> Tensor:
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).float().cpu()
        assert bool((g == SENT).all()), f"{what}: a guard element next to the output was written"
        assert not bool(self.t.isnan().any()), f"{what}: {int(self.t.isnan().sum())} of {self.t.numel()} elements were left unwritten (NaN)"
        return self.t

    def untouched(self, old: Tensor | None = None) -> bool:
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).float().cpu()
        body = self.t.float().cpu()
        return bool((g == SENT).all()) and (bool(body.isnan().all()) if old is None else torch.equal(body.double(), old.double().reshape(body.shape)))


def put(t: Tensor, dtype, dev) -> Tensor:
    """the float64 fixture ``t`` in ``dtype`` on ``dev``; the conversion is exact (asserted)"""
    v = t.to(dtype)
    assert torch.equal(v.double(), t), "a fixture value is not a number of the storage type"
    return v.to(dev).contiguous()


def is_bf16(t: Tensor) -> bool:
    return torch.equal(t.float().bfloat16().double(), t.double())


def budget(*mags: Tensor) -> float:
    """the largest sum of magnitudes among the reductions given; must stay below 2^24"""
    m = max(float(x.max()) for x in mags if x.numel())
    assert m < LIMIT, f"a reduction's sum of magnitudes {m} is not below 2^24"
    return m


def equal_chunked(got: Tensor, ref_rows, rows: int, what: str, step: int = 1 << 16) -> None:
    """got [rows, n] against ref_rows(a, b) -> float64 [b - a, n], ``step`` rows at a time"""
    for a in range(0, rows, step):
        b = min(a + step, rows)
        assert_equal(got[a:b], ref_rows(a, b), f"{what} rows {a} .. {b}")


# ------------------------------------------------------------------------------------------------ the entry points
class LibEntry:
    """the library's entry points, taking tensors; every method returns the C-ABI's return code"""

    def __init__(self, lib):
        from viscy_amd import _lib
        self._lib, self._m = lib, _lib

    def _call(self, name, *args):
        a = [self._m.ptr(x) if (x is None or isinstance(x, Tensor)) else x for x in args]
        rc = getattr(self._lib, name)(*a, self._m.stream())
        torch.cuda.synchronize()
        return rc

    def _ws(self, op, B, n, C, K, dev):
        want = ws_floats(op, B, n, C, K)
        said = self._lib.vsx_narrow_ws_floats(op, B, n, C, K)
        assert said == want, f"vsx_narrow_ws_floats(op {op}, B {B}, n {n}, C {C}, K {K}) = {said}, the restated grid needs {want}"
        return Guarded(want, F32, dev)

    def _reduced(self, name, ws, rc):
        if rc == 0:
            ws.check(name + " scratch (one partial per workgroup of the restated grid)")
        return rc

    def _code(self, t):
        return self._m.dtype_code(t.dtype)

    def stem_fwd(self, x, W, bias, out, kernel):
        B, Cin, Z, H, Wd = x.shape
        return self._call("vsx_narrow_stem_fwd", x, W, bias, out, B, Cin, Z, H, Wd, *kernel, W.shape[0], self._code(out))

    def stem_wgrad(self, x, df, dW, db, kernel):
        B, Cin, Z, H, Wd = x.shape
        C0, K = df.shape[1], Cin * math.prod(kernel)
        ws = self._ws(OP_STEM, B, df.shape[0], C0, K, x.device)
        return self._reduced("stem_wgrad", ws, self._call("vsx_narrow_stem_wgrad", x, df, dW, db, ws.t, ws.t.numel(), B, Cin, Z, H, Wd, *kernel,
                                                          C0, self._code(df)))

    def proj_fwd(self, cat, gamma, beta, Wp, bp, out, mean, rstd, eps=EPS):
        M, Ccat = cat.shape
        return self._call("vsx_narrow_proj_fwd", cat, gamma, beta, Wp, bp, out, mean, rstd, M, Ccat, out.shape[1], eps, self._code(cat))

    def proj_bwd(self, dout, cat, mean, rstd, gamma, beta, Wp, dxn, dW, db):
        M, Ccat = cat.shape
        C = dout.shape[1]
        ws = self._ws(OP_PROJ, 1, M, C, Ccat, cat.device)
        return self._reduced("proj_bwd", ws, self._call("vsx_narrow_proj_bwd", dout, cat, mean, rstd, gamma, beta, Wp, dxn, dW, db, ws.t,
                                                        ws.t.numel(), M, Ccat, C, self._code(cat)))

    def block_fwd1(self, x, dw_w, dw_b, W1f, b1f, y, colsq, B, H, W):
        C = x.shape[1]
        ws = self._ws(OP_FWD1, B, H * W, C, 0, x.device)
        return self._reduced("block_fwd1", ws, self._call("vsx_narrow_block_fwd1", x, dw_w, dw_b, W1f, b1f, y, colsq, ws.t, ws.t.numel(), B, H, W,
                                                          C, self._code(x)))

    def block_fwd2(self, y, x, W1f, b1f, s, gb, W2, b2, out, B, H, W):
        return self._call("vsx_narrow_block_fwd2", y, x, W1f, b1f, s, gb, W2, b2, out, B, H, W, x.shape[1], self._code(x))

    def block_bwd_a(self, dout, y, W1f, b1f, s, gb, W2, dW2, db2, P, S, B, H, W):
        C = y.shape[1]
        ws = self._ws(OP_BWD_A, B, H * W, C, 0, y.device)
        return self._reduced("block_bwd_a", ws, self._call("vsx_narrow_block_bwd_a", dout, y, W1f, b1f, s, gb, W2, dW2, db2, P, S, ws.t,
                                                           ws.t.numel(), B, H, W, C, self._code(y)))

    def block_bwd_b(self, dout, y, W1f, b1f, s, t, W2, dy, dW1f, db1f, B, H, W):
        C = y.shape[1]
        ws = self._ws(OP_BWD_B, B, H * W, C, 0, y.device)
        return self._reduced("block_bwd_b", ws, self._call("vsx_narrow_block_bwd_b", dout, y, W1f, b1f, s, t, W2, dy, dW1f, db1f, ws.t,
                                                           ws.t.numel(), B, H, W, C, self._code(y)))

    def block_bwd_c(self, dy, x, dout, dw_w, dx, ddw, ddb, B, H, W):
        C = x.shape[1]
        ws = self._ws(OP_BWD_C, B, H * W, C, 0, x.device)
        return self._reduced("block_bwd_c", ws, self._call("vsx_narrow_block_bwd_c", dy, x, dout, dw_w, dx, ddw, ddb, ws.t, ws.t.numel(), B, H, W,
                                                           C, self._code(x)))

    def shuffle_bwd(self, dout, dfeat, B, h, w, Cout, D, s, pool):
        return self._call("vsx_narrow_voxel_shuffle_bwd", dout, dfeat, B, h, w, Cout, D, s, int(pool), self._code(dfeat))


DEFECTS = ("ddw_last_tile_left_out", "second_tile_skipped", "s_of_sample_0", "bwd_c_taps_transposed", "proj_k176_dropped",
           "stem_row_tail_dropped", "pool_right_edge_unclipped")


def nchw(t: Tensor, B, H, W) -> Tensor:
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


def rows_of(t: Tensor) -> Tensor:
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def taps_to_conv(dw_w: Tensor) -> Tensor:
    """[49, C] (tap-major) -> the depthwise Conv2d weight [C, 1, 7, 7]"""
    return dw_w.t().reshape(-1, 1, 7, 7)


def patches(x: Tensor, kernel) -> Tensor:
    """[B, Cin, kz, H, W] -> [B h w, Cin kz ky kx] in the Conv3d weight order"""
    B, Cin, Z, H, W = x.shape
    kz, ky, kx = kernel
    h, w = H // ky, W // kx
    return x.view(B, Cin, kz, h, ky, w, kx).permute(0, 3, 5, 1, 2, 4, 6).reshape(B * h * w, Cin * kz * ky * kx)


class TorchEntry:
    """plain PyTorch (fp32, CPU) of the ten entry points with the rounding points of narrow.hip and none of its tiling: no tiles,
    no workgroups, no partials.  The admission checks of the C-ABI are restated.  ``defect`` seeds one indexing error (DEFECTS)."""

    def __init__(self, defect: str | None = None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    # -- stem
    def stem_fwd(self, x, W, bias, out, kernel):
        B, Cin, Z, H, Wd = x.shape
        C0, K = W.shape[0], Cin * math.prod(kernel)
        if Z != kernel[0] or H % kernel[1] or Wd % kernel[2] or C0 % vec_elems(out.dtype) or K * C0 + C0 > 16384:
            return 1
        out.copy_((bias + patches(x, kernel) @ W.reshape(C0, K).t()).to(out.dtype))
        return 0

    def stem_wgrad(self, x, df, dW, db, kernel):
        B, Cin, Z, H, Wd = x.shape
        C0, K = df.shape[1], Cin * math.prod(kernel)
        if Z != kernel[0] or H % kernel[1] or Wd % kernel[2] or C0 > 128 or K > 64 or C0 * (K + 1) > STEM_EPT * NB:
            return 1
        P, d = patches(x, kernel), df.float()
        if self.defect == "stem_row_tail_dropped":
            keep = d.shape[0] // STEM_ROWS * STEM_ROWS
            P, d = P[:keep], d[:keep]
        dW += (d.t() @ P).view_as(dW)
        db += d.sum(0)
        return 0

    # -- projection
    def _xn(self, cat, mean, rstd, gamma, beta):
        return ((cat.float() - mean[:, None]) * rstd[:, None]) * gamma + beta

    def proj_fwd(self, cat, gamma, beta, Wp, bp, out, mean, rstd, eps=EPS):
        M, Ccat = cat.shape
        C = out.shape[1]
        if C not in (4, 8) or Ccat > 16 * PJ_V:
            return 1
        v = cat.float()
        inv = torch.tensor(1.0) / torch.tensor(float(Ccat))
        mu = v.sum(1) * inv
        d = v - mu[:, None]
        rs = torch.rsqrt((d * d).sum(1) * inv + torch.tensor(eps))
        xn = self._xn(cat, mu, rs, gamma, beta)
        if self.defect == "proj_k176_dropped":
            xn[:, 176:] = 0.0
        out.copy_((xn @ Wp.reshape(C, Ccat).t() + bp).to(out.dtype))
        if mean is not None:
            mean.copy_(mu)
        rstd.copy_(rs)
        return 0

    def proj_bwd(self, dout, cat, mean, rstd, gamma, beta, Wp, dxn, dW, db):
        M, Ccat = cat.shape
        C = dout.shape[1]
        if C not in (4, 8) or Ccat > 16 * PJ_V:
            return 1
        d, xn = dout.float(), self._xn(cat, mean, rstd, gamma, beta)
        ke = min(Ccat, 176) if self.defect == "proj_k176_dropped" else Ccat
        dW.view(C, Ccat)[:, :ke] += (d.t() @ xn)[:, :ke]
        db += d.sum(0)
        dxn[:, :ke] = (d @ Wp.reshape(C, Ccat))[:, :ke].to(dxn.dtype)
        return 0

    # -- block
    def _live(self, B, H, W) -> Tensor:
        """the pixels a pass visits: all of them"""
        hw = H * W
        live = torch.ones(hw, dtype=torch.bool)
        tpw = blk_grid(B, hw)[1]
        if self.defect == "second_tile_skipped" and tpw > 1:
            live = (torch.arange(hw) // NB) % tpw != 1
        return live.repeat(B)

    def _s(self, s, hw):
        if self.defect == "s_of_sample_0":
            s = s[:1].expand_as(s)
        return s.repeat_interleave(hw, 0)

    @staticmethod
    def _hidden(y, W1f, b1f):
        C = y.shape[1]
        v = y.float()
        mu = v.sum(1, keepdim=True) * (1.0 / C)
        d = v - mu
        rs = torch.rsqrt((d * d).sum(1, keepdim=True) * (1.0 / C) + 1e-6)
        xh = d * rs
        return xh, rs, b1f + xh @ W1f.float().t()

    @staticmethod
    def _gelu(h):
        return 0.5 * h * (1.0 + torch.erf(h * RSQRT2))

    @staticmethod
    def _gelu_grad(h):
        return 0.5 * (1.0 + torch.erf(h * RSQRT2)) + h * RSQRT2PI * torch.exp(-0.5 * h * h)

    def block_fwd1(self, x, dw_w, dw_b, W1f, b1f, y, colsq, B, H, W):
        live = self._live(B, H, W)
        yv = rows_of(F.conv2d(nchw(x.float(), B, H, W), taps_to_conv(dw_w), dw_b, padding=3, groups=x.shape[1])).to(y.dtype)
        y[live] = yv[live]
        g = self._gelu(self._hidden(yv, W1f, b1f)[2]) * live[:, None]
        colsq += (g * g).view(B, H * W, -1).sum(1)
        return 0

    def block_fwd2(self, y, x, W1f, b1f, s, gb, W2, b2, out, B, H, W):
        live = self._live(B, H, W)
        z = self._gelu(self._hidden(y, W1f, b1f)[2]) * self._s(s, H * W) + gb
        o = (x.float() + b2 + z @ W2.float().t()).to(out.dtype)
        out[live] = o[live]
        return 0

    def block_bwd_a(self, dout, y, W1f, b1f, s, gb, W2, dW2, db2, P, S, B, H, W):
        live = self._live(B, H, W)[:, None]
        g = self._gelu(self._hidden(y, W1f, b1f)[2])
        z = (g * self._s(s, H * W) + gb) * live
        d = dout.float() * live
        dz = d @ W2.float()
        dW2 += d.t() @ z
        db2 += d.sum(0)
        P += (dz * g).view(B, H * W, -1).sum(1)
        S += dz.view(B, H * W, -1).sum(1)
        return 0

    def block_bwd_b(self, dout, y, W1f, b1f, s, t, W2, dy, dW1f, db1f, B, H, W):
        live = self._live(B, H, W)
        C = y.shape[1]
        xh, rs, h = self._hidden(y, W1f, b1f)
        dz = dout.float() @ W2.float()
        dh = (dz * self._s(s, H * W) + t.repeat_interleave(H * W, 0) * self._gelu(h)) * self._gelu_grad(h)
        dxh = dh @ W1f.float()
        m1, m2 = dxh.sum(1, keepdim=True) * (1.0 / C), (dxh * xh).sum(1, keepdim=True) * (1.0 / C)
        o = (rs * (dxh - m1 - xh * m2)).to(dy.dtype)
        dy[live] = o[live]
        dh = dh * live[:, None]
        dW1f += dh.t() @ xh
        db1f += dh.sum(0)
        return 0

    def block_bwd_c(self, dy, x, dout, dw_w, dx, ddw, ddb, B, H, W):
        live = self._live(B, H, W)
        C, hw = x.shape[1], H * W
        d4, x4 = nchw(dy.float(), B, H, W), nchw(x.float(), B, H, W)
        wt = taps_to_conv(dw_w)
        if self.defect == "bwd_c_taps_transposed":
            wt = wt.transpose(2, 3)
        o = (rows_of(F.conv2d(d4, wt.flip(2, 3), None, padding=3, groups=C)) + dout.float()).to(dx.dtype)
        dx[live] = o[live]
        dl = dy.float() * live[:, None]
        ddb += dl.sum(0)
        if self.defect == "ddw_last_tile_left_out" and hw % NB:
            dl = dl * ((torch.arange(hw) < hw // NB * NB).repeat(B))[:, None]
        d4, xp = nchw(dl, B, H, W), F.pad(x4, (3, 3, 3, 3))
        for tap in range(49):
            ky, kx = divmod(tap, 7)
            ddw[tap] += (d4 * xp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3))
        return 0

    # -- head adjoint
    def shuffle_bwd(self, dout, dfeat, B, h, w, Cout, D, s, pool):
        H, W = h * s, w * s
        d = dout.reshape(B * Cout * D, H * W).float()
        nt = s if pool else 1
        inv = torch.tensor(1.0) / torch.tensor(float(s * s)) if pool else torch.tensor(1.0)
        Y, X = torch.arange(H)[:, None], torch.arange(W)[None, :]
        acc = torch.zeros(B * Cout * D, H, W)
        for ty in range(nt):
            for tx in range(nt):
                ok = (Y + ty < H) & ((X + tx < W) | (self.defect == "pool_right_edge_unclipped"))
                idx = ((Y + ty) * W + X + tx).clamp_max(H * W - 1)
                acc += torch.where(ok, d[:, idx], torch.zeros(()))
        f = (acc * inv).view(B, Cout * D, h, s, w, s).permute(0, 2, 4, 1, 3, 5).reshape(B * h * w, Cout * D * s * s)
        dfeat.copy_(f.to(dfeat.dtype))
        return 0


# ------------------------------------------------------------------------------------------------ stem
def stem_cases():
    out = []

    def case(name, geo, kernel, Cin, C0, why, fwd=True, wgrad=True, dts=("fp32", "bf16"), chunk=False):
        B, h, w = geo
        K, M0 = Cin * math.prod(kernel), B * h * w
        rpw = stem_rows_per_wg(M0)
        leg = f"{why}: K = {K}, {M0} rows, rows_per_wg = {rpw}, {cdiv(M0, rpw)} workgroups, last one {M0 - (cdiv(M0, rpw) - 1) * rpw} rows"
        out.append(dict(name=name, B=B, h=h, w=w, kernel=kernel, Cin=Cin, C0=C0, K=K, M0=M0, fwd=fwd, wgrad=wgrad, dts=dts, leg=leg))

    for kname, kernel, Cin in (("k122", (1, 2, 2), 1), ("k522", (5, 2, 2), 1), ("k122_cin3", (1, 2, 2), 3)):
        case(f"{kname}_1x1x1", (1, 1, 1), kernel, Cin, 96, "a single patch")
        case(f"{kname}_3x13x21", (3, 13, 21), kernel, Cin, 96, "819 rows: a 51-row tail of the 64-row step")
        case(f"{kname}_1x257x256", (1, 257, 256), kernel, Cin, 96, "more than 65536 rows: 128 rows per workgroup, two 64-row steps each")
        case(f"{kname}_1x257x257", (1, 257, 257), kernel, Cin, 96, "128 rows per workgroup and a last workgroup of one row")
    case("limit_c128_k31", (2, 3, 5), (31, 1, 1), 1, 128, "C0 (K + 1) = 4096: the last STEM_EPT slot of every thread", fwd=False)
    case("limit_c63_k64", (2, 3, 5), (1, 8, 8), 1, 63, "K = 64 fills the patch tile, odd C0", fwd=False)
    case("lds_k15_c1024", (2, 3, 5), (1, 3, 5), 1, 1024, "K C0 + C0 = 16384 floats: 64 KB of dynamic LDS", wgrad=False)
    case("stride_1x700x1000", (1, 700, 1000), (1, 2, 2), 1, 96, "700000 x 24 = 16.8 M work items > 65536 x 256: the grid-stride loop runs twice",
         wgrad=False, dts=("fp32",))
    return out


def stem_refusals():
    """one past each admission limit: (name, entry, kernel, C0 by dtype)"""
    return [("fwd_lds", "fwd", (1, 3, 5), {"fp32": 1028, "bf16": 1032}), ("fwd_vector", "fwd", (1, 2, 2), {"fp32": 98, "bf16": 98}),
            ("wgrad_c129", "wgrad", (1, 1, 1), {"fp32": 129, "bf16": 129}), ("wgrad_k65", "wgrad", (65, 1, 1), {"fp32": 1, "bf16": 1}),
            ("wgrad_slots", "wgrad", (32, 1, 1), {"fp32": 128, "bf16": 128})]


_FIX: dict = {}


def clear_fixtures() -> None:
    _FIX.clear()


def _fixture(key, make):
    if key not in _FIX:
        _FIX[key] = make()
    return _FIX[key]


def stem_fixture(case) -> dict:
    def make():
        B, h, w, (kz, ky, kx), Cin, C0, K = (case[k] for k in ("B", "h", "w", "kernel", "Cin", "C0", "K"))
        s0 = _seed(case["name"])
        fx = dict(x=ints((B, Cin, kz, h * ky, w * kx), -1, 1, s0 + 1), W=ints((C0, K), -2, 2, s0 + 2), b=ints((C0,), -3, 3, s0 + 3))
        fx["P"] = patches(fx["x"], case["kernel"])
        budget(fx["b"].abs() + fx["W"].abs().sum(1))   # |patch| <= 1
        assert 3 + 2 * K <= 256   # every forward value is an integer a bf16 holds
        if case["wgrad"]:
            fx["df"] = ints((case["M0"], C0), -2, 2, s0 + 4)
            fx["dW0"], fx["db0"] = ints((C0, K), -4, 4, s0 + 5), ints((C0,), -4, 4, s0 + 6)
            fx["dW"], fx["db"] = fx["dW0"] + fx["df"].t() @ fx["P"], fx["db0"] + fx["df"].sum(0)
            budget(fx["dW0"].abs() + fx["df"].abs().t() @ fx["P"].abs(), fx["db0"].abs() + fx["df"].abs().sum(0))
        return fx
    return _fixture(("stem", case["name"]), make)


def run_stem_case(ep, case, dtn, dev) -> None:
    dt, fx, name, kernel = DTYPES[dtn], stem_fixture(case), case["name"], case["kernel"]
    x, C0, K, M0 = put(fx["x"], F32, dev), case["C0"], case["K"], case["M0"]
    if case["fwd"]:
        out = Guarded((M0, C0), dt, dev)
        shape = (C0, case["Cin"], *kernel)
        rc = ep.stem_fwd(x, put(fx["W"], F32, dev).view(shape), put(fx["b"], F32, dev), out.t, kernel)
        assert rc == 0, f"stem_fwd {name} {dtn}: return code {rc} ({case['leg']})"
        Wt, b = fx["W"].t().contiguous(), fx["b"]
        equal_chunked(out.check(f"stem_fwd {name} {dtn}"), lambda a, e: fx["P"][a:e] @ Wt + b, M0, f"stem_fwd {name} {dtn}")
    if case["wgrad"]:
        dW, db = Guarded((C0, K), F32, dev, fx["dW0"]), Guarded((C0,), F32, dev, fx["db0"])
        rc = ep.stem_wgrad(x, put(fx["df"], dt, dev), dW.t, db.t, kernel)
        assert rc == 0, f"stem_wgrad {name} {dtn}: return code {rc}"
        assert_equal(dW.check(f"stem_wgrad {name} {dtn} dW"), fx["dW"], f"stem_wgrad {name} {dtn} dW [C0, K] (+ old) ({case['leg']})")
        assert_equal(db.check(f"stem_wgrad {name} {dtn} db"), fx["db"], f"stem_wgrad {name} {dtn} db (+ old)")


def run_stem_refusal(ep, ref, dtn, dev) -> None:
    name, entry, kernel, c0 = ref
    dt, C0, K = DTYPES[dtn], c0[dtn], math.prod(kernel)
    B, h, w = 1, 2, 3
    x = put(ints((B, 1, kernel[0], h * kernel[1], w * kernel[2]), -1, 1, 5), F32, dev)
    if entry == "fwd":
        out = Guarded((B * h * w, C0), dt, dev)
        rc = ep.stem_fwd(x, torch.ones((C0, 1, *kernel), dtype=F32, device=dev), torch.ones(C0, dtype=F32, device=dev), out.t, kernel)
        assert rc != 0 and out.untouched(), f"stem_fwd {name} {dtn}: C0 = {C0}, K = {K} must be refused (rc {rc}) and the output left alone"
    else:
        old = ints((C0, K + 1), -4, 4, 6)
        dW, db = Guarded((C0, K), F32, dev, old[:, :K]), Guarded((C0,), F32, dev, old[:, K])
        rc = ep.stem_wgrad(x, torch.ones((B * h * w, C0), dtype=dt, device=dev), dW.t, db.t, kernel)
        assert rc != 0 and dW.untouched(old[:, :K]) and db.untouched(old[:, K]), \
            f"stem_wgrad {name} {dtn}: C0 = {C0}, K = {K} must be refused (rc {rc}) and the gradients left alone"


# ------------------------------------------------------------------------------------------------ projection
PROJ_M = (1, 15, 16, 17, 16385)
PROJ_CCAT = (1, 15, 17, 144, 191, 192)
PROJ_BIG = dict(M=1048577, Ccat=17, C=4)


def proj_fixture(M: int, Ccat: int, C: int, bwd: bool = True) -> dict:
    def make():
        s0 = _seed(f"proj{M}x{Ccat}x{C}")
        fx = dict(cat=ints((M, Ccat), -4, 4, s0 + 1), beta=ints((Ccat,), -1, 1, s0 + 2), W=ints((C, Ccat), -1, 1, s0 + 3), bp=ints((C,), -3, 3, s0 + 4))
        S = fx["cat"].sum(1)
        budget(fx["cat"].abs().sum(1), fx["bp"].abs() + fx["W"].abs() @ fx["beta"].abs())
        fx["mean"] = (S.float() * (torch.tensor(1.0) / torch.tensor(float(Ccat)))).double()   # fl(S fl(1 / Ccat)), S exact
        fx["out"] = (fx["bp"] + fx["W"] @ fx["beta"])[None].expand(M, C)                      # gamma = 0: xn == beta
        assert is_bf16(fx["out"])
        var = ((fx["cat"] - fx["cat"].mean(1, keepdim=True)) ** 2).mean(1)
        fx["rstd"] = torch.rsqrt(var + EPS).float().double()
        if bwd:
            fx["d"] = ints((M, C), -2, 2, s0 + 5)
            fx["dW0"], fx["db0"] = ints((C, Ccat), -4, 4, s0 + 6), ints((C,), -4, 4, s0 + 7)
            D = fx["d"].sum(0)
            fx["dxn"] = fx["d"] @ fx["W"]
            fx["dW"], fx["db"] = fx["dW0"] + D[:, None] * fx["beta"][None], fx["db0"] + D
            budget(fx["dW0"].abs() + fx["d"].abs().sum(0)[:, None] * fx["beta"].abs()[None], fx["db0"].abs() + fx["d"].abs().sum(0))
            assert is_bf16(fx["dxn"])
        return fx
    return _fixture(("proj", M, Ccat, C, bwd), make)


def run_proj_case(ep, M, Ccat, C, dtn, dev, bwd=True) -> None:
    dt, fx, what = DTYPES[dtn], proj_fixture(M, Ccat, C, bwd), f"M = {M}, Ccat = {Ccat}, C = {C}, {dtn}, gamma = 0"
    f = lambda k: put(fx[k], F32, dev)   # noqa: E731
    cat, gamma = put(fx["cat"], dt, dev), torch.zeros(Ccat, dtype=F32, device=dev)
    out, mean, rstd = Guarded((M, C), dt, dev), Guarded((M,), F32, dev), Guarded((M,), F32, dev)
    rc = ep.proj_fwd(cat, gamma, f("beta"), f("W"), f("bp"), out.t, mean.t, rstd.t)
    assert rc == 0, f"proj_fwd {what}: return code {rc}"
    equal_chunked(out.check("proj_fwd out " + what), lambda a, e: fx["out"][a:e], M, "proj_fwd out = bp + W beta " + what)
    assert_equal(mean.check("proj_fwd mean " + what), fx["mean"], "proj_fwd mean = fl(S fl(1 / Ccat)) " + what)
    rstd.check("proj_fwd rstd " + what)
    if bwd:
        dxn, dW, db = Guarded((M, Ccat), dt, dev), Guarded((C, Ccat), F32, dev, fx["dW0"]), Guarded((C,), F32, dev, fx["db0"])
        rc = ep.proj_bwd(put(fx["d"], dt, dev), cat, f("mean"), f("rstd"), gamma, f("beta"), f("W"), dxn.t, dW.t, db.t)
        assert rc == 0, f"proj_bwd {what}: return code {rc}"
        assert_equal(dxn.check("proj_bwd dxn " + what), fx["dxn"], "proj_bwd dxn " + what)
        assert_equal(dW.check("proj_bwd dW " + what), fx["dW"], "proj_bwd dW = old + beta[k] sum_r d[r, c] " + what)
        assert_equal(db.check("proj_bwd db " + what), fx["db"], "proj_bwd db " + what)


def run_proj_refusal(ep, C, dtn, dev) -> None:
    dt, M, Ccat = DTYPES[dtn], 3, 16 * PJ_V + 1
    z = lambda *s, d=F32: torch.ones(s, dtype=d, device=dev)   # noqa: E731
    out, mean, rstd, dxn = Guarded((M, C), dt, dev), Guarded((M,), F32, dev), Guarded((M,), F32, dev), Guarded((M, Ccat), dt, dev)
    rc = ep.proj_fwd(z(M, Ccat, d=dt), z(Ccat), z(Ccat), z(C, Ccat), z(C), out.t, mean.t, rstd.t)
    assert rc != 0 and out.untouched() and mean.untouched() and rstd.untouched(), f"proj_fwd Ccat = {Ccat} must be refused (rc {rc})"
    old = ints((C, Ccat + 1), -4, 4, 9)
    dW, db = Guarded((C, Ccat), F32, dev, old[:, :Ccat]), Guarded((C,), F32, dev, old[:, Ccat])
    rc = ep.proj_bwd(z(M, C, d=dt), z(M, Ccat, d=dt), z(M), z(M), z(Ccat), z(Ccat), z(C, Ccat), dxn.t, dW.t, db.t)
    assert rc != 0 and dxn.untouched() and dW.untouched(old[:, :Ccat]) and db.untouched(old[:, Ccat]), f"proj_bwd Ccat = {Ccat} must be refused (rc {rc})"


# ------------------------------------------------------------------------------------------------ shuffle adjoint
SHUFFLE_CFG = ((1, 1, 2, True), (1, 1, 2, False), (2, 3, 2, True), (1, 1, 3, True), (1, 5, 1, False))
SHUFFLE_GEO = ((1, 1, 1), (2, 3, 5), (1, 64, 96))
SHUFFLE_BIG = ((1, 1, 2, True), (1, 2048, 2049))   # 2048 x 2049 x 4 = 16 785 408 elements > 65536 x 256


def shuffle_statement(dout: Tensor, B, h, w, Cout, D, s, pool, dt) -> Tensor:
    """float64 [B h w, Cout D s s]: the adjoint of pixel_shuffle(s) followed by the causal s x s mean (stride 1, zero padding on the
    left and top): the sum of dout over [Y, Y + s) x [X, X + s) clipped at the bottom and right, times fl(1 / s^2) in fp32"""
    H, W = h * s, w * s
    d = dout.reshape(B, Cout * D, H, W)
    if pool:
        p = F.pad(d, (0, s - 1, 0, s - 1))
        acc = sum(p[:, :, ty:ty + H, tx:tx + W] for ty in range(s) for tx in range(s))
        mag = sum(p[:, :, ty:ty + H, tx:tx + W].abs() for ty in range(s) for tx in range(s))
        budget(mag)
        inv = torch.tensor(1.0) / torch.tensor(float(s * s))
        v = acc.float() * inv
        if s & (s - 1) == 0:
            assert torch.equal(v.double(), acc / (s * s))   # a power of two: the product is exact
    else:
        v = d.float()
    v = rows_of(F.pixel_unshuffle(v, s))
    if dt == BF16:
        r = v.bfloat16()
        assert s == 3 or torch.equal(r.double(), v.double()), "a stored value is not a bf16 number"
        v = r
    return v.double()


def run_shuffle_case(ep, cfg, geo, dtn, dev) -> None:
    (Cout, D, s, pool), (B, h, w), dt = cfg, geo, DTYPES[dtn]
    what = f"voxel_shuffle_bwd (Cout, D, s, pool) = {cfg}, (B, h, w) = {geo}, {dtn}"
    dout = ints((B, Cout, D, h * s, w * s), -8, 8, _seed(f"shuffle{cfg}{geo}"))
    ref = shuffle_statement(dout, B, h, w, Cout, D, s, pool, dt)
    df = Guarded(ref.shape, dt, dev)
    rc = ep.shuffle_bwd(put(dout, F32, dev), df.t, B, h, w, Cout, D, s, pool)
    assert rc == 0, f"{what}: return code {rc}"
    equal_chunked(df.check(what), lambda a, e: ref[a:e], ref.shape[0], what, step=1 << 20)


# ------------------------------------------------------------------------------------------------ block passes: exact tier
BLOCK_SHAPES = ((1, 1, 1), (1, 3, 5), (1, 16, 16), (2, 7, 37), (3, 13, 21), (300, 8, 257), (2049, 3, 86))
BLOCK_WHY = {(1, 1, 1): "a single pixel", (1, 3, 5): "a map smaller than the window", (1, 16, 16): "exactly one full tile",
             (2, 7, 37): "259 pixels: a tile edge inside a row, a 3-pixel tail, a second sample", (3, 13, 21): "the shape of the tolerance tests",
             (300, 8, 257): "nt = 9, tpw = 2, gps = 5: the last workgroup has one tile of 8 pixels",
             (2049, 3, 86): "B > 2048, want = 1, tpw = 2, gps = 1: a 2-pixel second tile"}
BOUNDED_SHAPES = ((2, 7, 37), (1, 16, 16), (300, 8, 257))


def block_plan(shape) -> dict:
    B, H, W = shape
    hw = H * W
    nt = cdiv(hw, NB)
    gps, tpw = blk_grid(B, hw)
    return dict(nt=nt, gps=gps, tpw=tpw, last_tiles=nt - (gps - 1) * tpw, last_pixels=hw - (nt - 1) * NB)


def block_fixture(shape, C: int) -> dict:
    """integer operands of the five passes and their float64 statements; shared by both dtypes"""
    def make():
        B, H, W = shape
        hw, HD, s0 = H * W, 4 * C, _seed(f"block{shape}x{C}")
        M, big = B * hw, B * hw > 100000
        fx = dict(x=ints((M, C), -2, 2, s0 + 1), dw_w=ints((49, C), -2, 2, s0 + 2), dw_b=ints((C,), -3, 3, s0 + 3),
                  b1f=choice((16.0, -16.0, 32.0, -32.0), (HD,), s0 + 4), W2=ints((C, HD), -1, 1, s0 + 5), b2=16.0 * ints((C,), -2, 2, s0 + 6),
                  gb=16.0 * ints((HD,), -1, 1, s0 + 7), x2=16.0 * ints((M, C), -2, 2, s0 + 8), dyc=ints((M, C), -1, 1, s0 + 9))
        fx["b1f"][:4] = torch.tensor([16.0, -16.0, 32.0, -32.0])   # all four values in every fixture
        sparse = (0.0, 0.0, 0.0, 1.0, -1.0)
        fx["s"] = choice(sparse, (B, HD), s0 + 10) if big else ints((B, HD), -2, 2, s0 + 10)
        fx["t"] = choice(sparse, (B, HD), s0 + 11) if big else ints((B, HD), -2, 2, s0 + 11)
        fx["dout"] = choice((-1.0, 0.0, 0.0, 1.0), (M, C), s0 + 12) if big else ints((M, C), -2, 2, s0 + 12)
        assert B == 1 or not torch.equal(fx["s"][0], fx["s"][1]), "s must differ between samples"
        old = lambda *sh, k: ints(sh, 1, 9, s0 + 20 + k)   # noqa: E731
        fx["old"] = dict(cs=old(B, HD, k=0), dW2=old(C, HD, k=1), db2=old(C, k=2), P=old(B, HD, k=3), S=old(B, HD, k=4), dW1f=old(HD, C, k=5),
                         db1f=old(HD, k=6), ddw=old(49, C, k=7), ddb=old(C, k=8))
        o = fx["old"]
        # pass 1: the depthwise output, and n b1f^2 per sample where b1f > 0
        x4, wt = nchw(fx["x"], B, H, W), taps_to_conv(fx["dw_w"])
        fx["y"] = rows_of(F.conv2d(x4, wt, fx["dw_b"], padding=3, groups=C))
        budget(rows_of(F.conv2d(x4.abs(), wt.abs(), fx["dw_b"].abs(), padding=3, groups=C)))
        g = fx["b1f"].clamp_min(0.0)
        pos = (fx["b1f"] > 0).double()
        fx["cs"] = o["cs"] + hw * g * g
        budget(fx["cs"])
        # pass 2: z[b, j] = g[j] s[b, j] + gb[j] for every pixel of sample b
        z = g * fx["s"] + fx["gb"]
        fx["out"] = fx["x2"] + fx["b2"] + (z @ fx["W2"].t()).repeat_interleave(hw, 0)
        budget(fx["x2"].abs().max() + fx["b2"].abs() + z.abs() @ fx["W2"].abs().t())
        # pass A
        Db, Da = fx["dout"].view(B, hw, C).sum(1), fx["dout"].abs().view(B, hw, C).sum(1)
        Sb, Sa = Db @ fx["W2"], Da @ fx["W2"].abs()
        fx["dW2"], fx["db2"] = o["dW2"] + Db.t() @ z, o["db2"] + Db.sum(0)
        fx["S"], fx["P"] = o["S"] + Sb, o["P"] + Sb * g
        budget(o["dW2"] + Da.t() @ z.abs(), o["db2"] + Da.sum(0), o["S"] + Sa, o["P"] + Sa * g)
        # pass B: dh = (dz s + t g) [b1f > 0]
        fx["db1f"] = o["db1f"] + ((Sb * fx["s"] + hw * fx["t"] * g) * pos).sum(0)
        budget(o["db1f"] + (Sa * fx["s"].abs() + hw * fx["t"].abs() * g).sum(0))
        # pass C
        d4 = nchw(fx["dyc"], B, H, W)
        fx["dx"] = rows_of(F.conv2d(d4, wt.flip(2, 3), None, padding=3, groups=C)) + fx["dout"]
        xp = F.pad(x4, (3, 3, 3, 3))
        fx["ddw"] = o["ddw"] + torch.stack([(d4 * xp[:, :, ky:ky + H, kx:kx + W]).sum((0, 2, 3)) for ky in range(7) for kx in range(7)])
        fx["ddb"] = o["ddb"] + fx["dyc"].sum(0)
        budget(o["ddw"] + float((fx["dyc"].abs().sum(0) * 2).max()), o["ddb"] + fx["dyc"].abs().sum(0), 49.0 * 2 + fx["dout"].abs().max().reshape(1))
        for k in ("y", "out", "dx"):
            assert is_bf16(fx[k]), f"{k} holds a value that is not a bf16 number"
        return fx
    return _fixture(("block", shape, C), make)


def run_block_exact(ep, shape, C, dtn, dev) -> None:
    B, H, W = shape
    dt, fx, hw, HD = DTYPES[dtn], block_fixture(shape, C), H * W, 4 * C
    M, o = B * hw, fx["old"]
    tag = f"{shape} C = {C} {dtn} ({BLOCK_WHY[shape]})"
    f, d = (lambda k: put(fx[k], F32, dev)), (lambda k: put(fx[k], dt, dev))
    acc = lambda k: Guarded(o[k].shape, F32, dev, o[k])   # noqa: E731
    W1f = torch.zeros((HD, C), dtype=dt, device=dev)
    erf = " (exact only if erff(+-11.3) == +-1 on this device)"
    # pass 1
    y, cs = Guarded((M, C), dt, dev), acc("cs")
    rc = ep.block_fwd1(d("x"), f("dw_w"), f("dw_b"), W1f, f("b1f"), y.t, cs.t, B, H, W)
    assert rc == 0, f"block_fwd1 {tag}: return code {rc}"
    assert_equal(y.check("block_fwd1 y " + tag), fx["y"], "block_fwd1 y = dwconv7(x) + bias " + tag)
    assert_equal(cs.check("block_fwd1 colsq " + tag), fx["cs"], "block_fwd1 colsq = old + n b1f^2 [b1f > 0]" + erf + " " + tag)
    # pass 2
    out = Guarded((M, C), dt, dev)
    rc = ep.block_fwd2(d("y"), d("x2"), W1f, f("b1f"), f("s"), f("gb"), d("W2"), f("b2"), out.t, B, H, W)
    assert rc == 0, f"block_fwd2 {tag}: return code {rc}"
    assert_equal(out.check("block_fwd2 out " + tag), fx["out"], "block_fwd2 out = x + b2 + W2 (g s[b] + gb)" + erf + " " + tag)
    # pass A
    dW2, db2, P, S = acc("dW2"), acc("db2"), acc("P"), acc("S")
    rc = ep.block_bwd_a(d("dout"), d("y"), W1f, f("b1f"), f("s"), f("gb"), d("W2"), dW2.t, db2.t, P.t, S.t, B, H, W)
    assert rc == 0, f"block_bwd_a {tag}: return code {rc}"
    for k, buf in (("dW2", dW2), ("db2", db2), ("P", P), ("S", S)):
        assert_equal(buf.check(f"block_bwd_a {k} " + tag), fx[k], f"block_bwd_a {k} (+ old)" + (erf if k in ("dW2", "P") else "") + " " + tag)
    # pass B
    dy, dW1f, db1f = Guarded((M, C), dt, dev), acc("dW1f"), acc("db1f")
    rc = ep.block_bwd_b(d("dout"), d("y"), W1f, f("b1f"), f("s"), f("t"), d("W2"), dy.t, dW1f.t, db1f.t, B, H, W)
    assert rc == 0, f"block_bwd_b {tag}: return code {rc}"
    assert_equal(db1f.check("block_bwd_b db1f " + tag), fx["db1f"], "block_bwd_b db1f = old + sum (dz s + t g) [b1f > 0]" + erf + " " + tag)
    assert_equal(dy.check("block_bwd_b dy " + tag), torch.zeros((M, C), dtype=F64), "block_bwd_b dy == 0 with W1f = 0 " + tag)
    dW1f.check("block_bwd_b dW1f " + tag)
    # pass C
    dx, ddw, ddb = Guarded((M, C), dt, dev), acc("ddw"), acc("ddb")
    rc = ep.block_bwd_c(d("dyc"), d("x"), d("dout"), f("dw_w"), dx.t, ddw.t, ddb.t, B, H, W)
    assert rc == 0, f"block_bwd_c {tag}: return code {rc}"
    assert_equal(dx.check("block_bwd_c dx " + tag), fx["dx"], "block_bwd_c dx = dwconv7^T(dy) + dout " + tag)
    assert_equal(ddw.check("block_bwd_c ddw " + tag), fx["ddw"], "block_bwd_c ddw [49, C] (+ old) " + tag)
    assert_equal(ddb.check("block_bwd_c ddb " + tag), fx["ddb"], "block_bwd_c ddb (+ old) " + tag)


# ------------------------------------------------------------------------------------------------ bounded tier
def fn(x: RE, f, df, ulp: float) -> RE:
    """a library function of a computed argument: |err| <= |f'| k_x u A_x + ulp 2 u |f|"""
    v = f(x.v)
    return RE(v, torch.maximum(v.abs(), df(x.v).abs() * x.A * (x.k > 0)), x.k + int(2 * ulp))


def chain(terms) -> RE:
    """a sequential sum (each fma or addition rounds once)"""
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def re_hidden(y: Tensor, W1f: Tensor, b1f: Tensor):
    """ln_fc1 of narrow.hip on rows y [n, C]: xh (list of C RE [n]), rs (RE [n]), h (list of 4C RE [n])"""
    C = y.shape[1]
    yc = [RE(y[:, c]) for c in range(C)]
    mu = chain(yc) * RE(1.0 / C)
    d = [v - mu for v in yc]
    var = chain([x * x for x in d])
    rs = fn(var * RE(1.0 / C) + RE(f32c(1e-6)), lambda v: v.rsqrt(), lambda v: 0.5 * v.pow(-1.5), RSQRT_ULP)
    xh = [x * rs for x in d]
    h = [chain([RE(b1f[j])] + [RE(W1f[j, c]) * xh[c] for c in range(C)]) for j in range(W1f.shape[0])]
    return xh, rs, h


def _erf_part(h: RE) -> RE:
    c = f32c(RSQRT2)
    return RE(1.0) + fn(h * RE(c), torch.erf, lambda v: 2.0 / math.sqrt(math.pi) * torch.exp(-v * v), ERF_ULP)


def re_gelu(h: RE) -> RE:
    return (RE(0.5) * h) * _erf_part(h)


def re_gelu_grad(h: RE) -> RE:
    e = fn(RE(-0.5) * h * h, torch.exp, torch.exp, EXP_K / 2)
    return RE(0.5) * _erf_part(h) + h * RE(f32c(RSQRT2PI)) * e


def stack(rs: list) -> RE:
    """a list of RE [n] -> one RE [n, len]; the count is that of the longest path"""
    return RE(torch.stack([r.v for r in rs], 1), torch.stack([torch.broadcast_to(r.A, r.v.shape) for r in rs], 1), max(r.k for r in rs))


# rounded operations on the longest path, by C (block) or Ccat (projection) and output; derived by RE from the formulas above (the
# operands hold no zero and no power of two, so the count follows from the formulas alone), pinned here
K_BLOCK = {4: dict(xh=14, g2=55, z=56, dz=4, Pt=55, dh=57, out=73, dy=80), 8: dict(xh=22, g2=67, z=68, dz=8, Pt=67, dh=69, out=101, dy=112)}
K_PROJ = {17: dict(rstd=14, xn=17, out=24), 144: dict(rstd=21, xn=24, out=38), 192: dict(rstd=24, xn=27, out=44)}
PALETTE, VARIANTS = 256, 4


def odd8(shape, seed: int, den: float = 8.0, positive: bool = False) -> Tensor:
    """k / den with k in {3, 5, 6, 7} (and their negatives): no zero, no power of two, three significant bits"""
    vals = (3.0, 5.0, 6.0, 7.0) + (() if positive else (-3.0, -5.0, -6.0, -7.0))
    return choice(vals, shape, seed) / den


def take(r: RE, idx: Tensor) -> RE:
    return RE(r.v[idx], r.A[idx], r.k)


def bounded_fixture(shape, C: int) -> dict:
    """dyadic operands (multiples of 1/8 or 1/64 with at most 6 significant bits: exact in fp32 and bf16) and the RE statements.
    A pixel's outputs depend on its own row of y / dout / x and on its sample's s / t alone, so the maps are drawn from a palette of
    PALETTE rows and the samples from VARIANTS vectors (sample b has vector b % VARIANTS): the statement is evaluated once per
    (vector, palette row) and gathered, which keeps the 616 800-pixel shape affordable."""
    def make():
        B, H, W = shape
        hw, HD, s0 = H * W, 4 * C, _seed(f"bounded{shape}x{C}")
        M, Q, V = B * hw, PALETTE, min(B, VARIANTS)
        q8 = lambda sh, k: ints(sh, -16, 16, s0 + k) / 8.0   # noqa: E731
        pal = dict(y=q8((Q, C), 1), x2=q8((Q, C), 2), dout=q8((Q, C), 3))
        fx = dict(W1f=odd8((HD, C), s0 + 4), b1f=odd8((HD,), s0 + 5), W2=odd8((C, HD), s0 + 6), b2=odd8((C,), s0 + 7), gb=odd8((HD,), s0 + 8))
        sV, tV = odd8((V, HD), s0 + 9, positive=True), odd8((V, HD), s0 + 10, den=64.0)
        y, x2, dout = (pal[k].repeat(V, 1) for k in ("y", "x2", "dout"))
        sb, tb = sV.repeat_interleave(Q, 0), tV.repeat_interleave(Q, 0)
        # |h| <= 4 (the range EXP_K is derived for): halve fc1 until the statement says so
        xh, rs, h = re_hidden(y, fx["W1f"], fx["b1f"])
        while max(float(r.v.abs().max()) for r in h) > 4.0:
            fx["W1f"], fx["b1f"] = fx["W1f"] / 2, fx["b1f"] / 2
            xh, rs, h = re_hidden(y, fx["W1f"], fx["b1f"])
        fx["hmax"] = max(float(r.v.abs().max()) for r in h)
        g = [re_gelu(x) for x in h]
        z = [g[j] * RE(sb[:, j]) + RE(fx["gb"][j]) for j in range(HD)]
        d = [RE(dout[:, c]) for c in range(C)]
        dz = [chain([d[c] * RE(fx["W2"][c, j]) for c in range(C)]) for j in range(HD)]
        dh = [(dz[j] * RE(sb[:, j]) + RE(tb[:, j]) * g[j]) * re_gelu_grad(h[j]) for j in range(HD)]
        dxh = [chain([dh[j] * RE(fx["W1f"][j, c]) for j in range(HD)]) for c in range(C)]
        m1 = chain(dxh) * RE(1.0 / C)
        m2 = chain([dxh[c] * xh[c] for c in range(C)]) * RE(1.0 / C)
        rows = dict(g2=stack([x * x for x in g]), z=stack(z), dz=stack(dz), Pt=stack([dz[j] * g[j] for j in range(HD)]), dh=stack(dh), xh=stack(xh),
                    out=stack([chain([RE(x2[:, c]) + RE(fx["b2"][c])] + [RE(fx["W2"][c, j]) * z[j] for j in range(HD)]) for c in range(C)]),
                    dy=stack([rs * (dxh[c] - m1 - xh[c] * m2) for c in range(C)]))
        fx["k"] = {k: r.k for k, r in rows.items()}
        pix, var = ints((B, hw), 0, Q - 1, s0 + 11).long(), torch.arange(B) % V
        idx = (var[:, None] * Q + pix).flatten()
        fx.update({k: take(r, idx) for k, r in rows.items()})
        fx.update({k: pal[k][pix.flatten()] for k in pal}, s=sV[var], t=tV[var])
        fx["old"] = {k: ints(sh, 1, 9, s0 + 30 + i) / 8.0 for i, (k, sh) in enumerate(
            dict(cs=(B, HD), dW2=(C, HD), db2=(C,), P=(B, HD), S=(B, HD), dW1f=(HD, C), db1f=(HD,)).items())}
        return fx
    return _fixture(("bounded", shape, C), make)


def _within(got: Tensor, r: RE, K: int, what: str, bf16: bool = False) -> float:
    """|got - v| <= K u A (+ U16 |v| for a bf16 store) per element; the worst err / bound"""
    assert r.k == K, f"{what}: the statement counts {r.k} rounded operations, the table says {K}"
    gv = got.detach().cpu().double().reshape(r.v.shape)
    bound = (K * U32 * r.A + (U16 * (r.v.abs() + K * U32 * r.A) if bf16 else 0.0)) * SLACK
    err = (gv - r.v).abs()
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    if not bool((err <= bound).all()):
        idx = (~(err <= bound)).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((~(err <= bound)).sum())} of {err.numel()} elements past the bound (worst {ratio:.3g} of it), first at {idx}: "
                             f"got {gv[tuple(idx)].item()!r}, statement {r.v[tuple(idx)].item()!r}")
    return ratio


def _sum_within(got: Tensor, old: Tensor, v: Tensor, A: Tensor, K: int, n: int, what: str) -> float:
    """a sum of n terms v (each within K u A of its statement), added to ``old``: (n + 1 + K) u (|old| + sum A)"""
    ref, mag = old + v, old.abs() + A
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    bound = (n + 1 + K) * U32 * mag * SLACK
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    assert bool((err <= bound).all()), f"{what}: worst error {ratio:.3g} of (n + K) u sum|v|, n = {n}, K = {K}"
    return ratio


def _prod_terms(a: RE, b: RE):
    """sum over rows of a[:, i] b[:, j]: values [I, J], the summed magnitudes of the products (RE's product rule, written with
    matrix products: A >= |v| makes |b| A_a + |a| A_b the larger term whenever a factor is computed) and the count of one product"""
    assert bool((a.A >= a.v.abs()).all()) and bool((b.A >= b.v.abs()).all()) and (a.k > 0 or b.k > 0)
    A = (a.k > 0) * (a.A.t() @ b.v.abs()) + (b.k > 0) * (a.v.abs().t() @ b.A)
    return a.v.t() @ b.v, A, max(a.k, b.k) + 1


def run_block_bounded(ep, shape, C, dtn, dev) -> None:
    B, H, W = shape
    dt, fx, hw, HD = DTYPES[dtn], bounded_fixture(shape, C), H * W, 4 * C
    M, o, K, bf = B * hw, fx["old"], K_BLOCK[C], DTYPES[dtn] == BF16
    tag = f"{shape} C = {C} {dtn}"
    f, d = (lambda k: put(fx[k], F32, dev)), (lambda k: put(fx[k], dt, dev))
    acc = lambda k: Guarded(o[k].shape, F32, dev, o[k])   # noqa: E731
    per = lambda t: t.view(B, hw, -1).sum(1)              # noqa: E731
    rec = {}
    # pass 1 on a depthwise filter that hands x through (centre tap 1): y == x, the GRN sums are the bounded output
    dw_w = torch.zeros((49, C), dtype=F32, device=dev)
    dw_w[24] = 1.0
    y, cs = Guarded((M, C), dt, dev), acc("cs")
    assert ep.block_fwd1(d("y"), dw_w, torch.zeros(C, dtype=F32, device=dev), d("W1f"), f("b1f"), y.t, cs.t, B, H, W) == 0
    assert_equal(y.check("block_fwd1 y " + tag), fx["y"], "block_fwd1 y through the centre tap " + tag)
    assert fx["g2"].k == K["g2"], f"g^2 counts {fx['g2'].k} operations, the table says {K['g2']}"
    rec["cs"] = _sum_within(cs.check("colsq " + tag), o["cs"], per(fx["g2"].v), per(fx["g2"].A), K["g2"], hw, "block_fwd1 colsq " + tag)
    # pass 2
    out = Guarded((M, C), dt, dev)
    assert ep.block_fwd2(d("y"), d("x2"), d("W1f"), f("b1f"), f("s"), f("gb"), d("W2"), f("b2"), out.t, B, H, W) == 0
    rec["out"] = _within(out.check("block_fwd2 out " + tag), fx["out"], K["out"], "block_fwd2 out " + tag, bf)
    # pass A
    dW2, db2, P, S = acc("dW2"), acc("db2"), acc("P"), acc("S")
    assert ep.block_bwd_a(d("dout"), d("y"), d("W1f"), f("b1f"), f("s"), f("gb"), d("W2"), dW2.t, db2.t, P.t, S.t, B, H, W) == 0
    assert fx["z"].k == K["z"] and fx["dz"].k == K["dz"], f"z / dz count {fx['z'].k} / {fx['dz'].k} operations, the table says {K['z']} / {K['dz']}"
    v, A, k = _prod_terms(RE(fx["dout"]), fx["z"])
    rec["dW2"] = _sum_within(dW2.check("dW2 " + tag), o["dW2"], v, A, k, M, "block_bwd_a dW2 " + tag)
    assert fx["Pt"].k == K["Pt"], f"dz g counts {fx['Pt'].k} operations, the table says {K['Pt']}"
    rec["P"] = _sum_within(P.check("P " + tag), o["P"], per(fx["Pt"].v), per(fx["Pt"].A), K["Pt"], hw, "block_bwd_a P " + tag)
    _sum_within(db2.check("db2 " + tag), o["db2"], fx["dout"].sum(0), fx["dout"].abs().sum(0), 0, M, "block_bwd_a db2 " + tag)
    _sum_within(S.check("S " + tag), o["S"], per(fx["dz"].v), per(fx["dz"].A), K["dz"], hw, "block_bwd_a S " + tag)
    # pass B
    dy, dW1f, db1f = Guarded((M, C), dt, dev), acc("dW1f"), acc("db1f")
    assert ep.block_bwd_b(d("dout"), d("y"), d("W1f"), f("b1f"), f("s"), f("t"), d("W2"), dy.t, dW1f.t, db1f.t, B, H, W) == 0
    rec["dy"] = _within(dy.check("block_bwd_b dy " + tag), fx["dy"], K["dy"], "block_bwd_b dy " + tag, bf)
    assert fx["dh"].k == K["dh"] and fx["xh"].k == K["xh"], f"dh / xh count {fx['dh'].k} / {fx['xh'].k} operations, the table says {K['dh']} / {K['xh']}"
    v, A, k = _prod_terms(fx["dh"], fx["xh"])
    rec["dW1f"] = _sum_within(dW1f.check("dW1f " + tag), o["dW1f"], v, A, k, M, "block_bwd_b dW1f " + tag)
    rec["db1f"] = _sum_within(db1f.check("db1f " + tag), o["db1f"], fx["dh"].v.sum(0), fx["dh"].A.sum(0), K["dh"], M, "block_bwd_b db1f " + tag)
    record(f"block/{B}x{H}x{W}/C{C}/{dtn}", **rec)


PROJ_BOUNDED = ((37, 17), (16385, 144), (33, 192))   # (M, Ccat) of the live-gamma statement


def proj_bounded_fixture(M: int, Ccat: int, C: int) -> dict:
    def make():
        s0 = _seed(f"projb{M}x{Ccat}x{C}")
        q = lambda sh, lo, hi, k, den=8.0: ints(sh, lo, hi, s0 + k) / den   # noqa: E731
        fx = dict(cat=q((M, Ccat), -16, 16, 1), gamma=odd8((Ccat,), s0 + 2, positive=True), beta=odd8((Ccat,), s0 + 3), W=odd8((C, Ccat), s0 + 4),
                  bp=odd8((C,), s0 + 5), d=q((M, C), -8, 8, 6), dW0=q((C, Ccat), 1, 9, 7))
        if Ccat > 1:
            fx["cat"][:, 0] = fx["cat"][:, 1] + 1.0   # no constant row: the variance stays above 1 / (4 Ccat)
        cat = fx["cat"]
        assert float(cat.abs().sum(1).max()) * 8 < LIMIT
        tree = lambda xs: xs[0] if len(xs) == 1 else tree([a + b for a, b in zip(xs[::2], xs[1::2])] + ([xs[-1]] if len(xs) % 2 else []))  # noqa: E731
        inv = RE(f32c(1.0 / Ccat)) if Ccat & (Ccat - 1) else RE(1.0 / Ccat)
        # the sums are exact (multiples of 1/8 below 2^24 / 8); only the product with fl(1 / Ccat) rounds
        S = cat.sum(1)
        mu = RE(S) * inv
        fx["mean"] = (S.float() * (torch.tensor(1.0) / torch.tensor(float(Ccat)))).double()
        dk = [RE(cat[:, k]) - mu for k in range(Ccat)]
        q_l = [chain([dk[k] * dk[k] for k in range(l, Ccat, 16)]) for l in range(min(16, Ccat))]
        var = tree(q_l) * inv + RE(f32c(EPS))
        rs = fn(var, lambda v: v.rsqrt(), lambda v: 0.5 * v.pow(-1.5), RSQRT_ULP)
        fx["rstd"] = rs
        xn = [dk[k] * rs * RE(fx["gamma"][k]) + RE(fx["beta"][k]) for k in range(Ccat)]
        fx["xn"] = stack(xn)
        outs = []
        for c in range(C):
            o_l = [chain([RE(fx["W"][c, k]) * xn[k] for k in range(l, Ccat, 16)]) for l in range(min(16, Ccat))]
            outs.append(tree(o_l) + RE(fx["bp"][c]))
        fx["out"] = stack(outs)
        return fx
    return _fixture(("projb", M, Ccat, C), make)


def run_proj_bounded(ep, M, Ccat, C, dtn, dev) -> None:
    """live gamma.  The backward re-forms xn from the statement's mean (the forward's bits) and its rstd rounded to fp32: one rounding
    of rstd, which the count of the forward's own rsqrtf path already covers"""
    dt, fx, bf = DTYPES[dtn], proj_bounded_fixture(M, Ccat, C), DTYPES[dtn] == BF16
    what = f"M = {M}, Ccat = {Ccat}, C = {C}, {dtn}"
    f = lambda k: put(fx[k], F32, dev)   # noqa: E731
    cat = put(fx["cat"], dt, dev)
    out, mean, rstd = Guarded((M, C), dt, dev), Guarded((M,), F32, dev), Guarded((M,), F32, dev)
    assert ep.proj_fwd(cat, f("gamma"), f("beta"), f("W"), f("bp"), out.t, mean.t, rstd.t) == 0
    assert_equal(mean.check("proj_fwd mean " + what), fx["mean"], "proj_fwd mean " + what)
    K = K_PROJ[Ccat]
    assert fx["xn"].k == K["xn"], f"xn counts {fx['xn'].k} operations, the table says {K['xn']}"
    rec = dict(rstd=_within(rstd.check("rstd " + what), fx["rstd"], K["rstd"], "proj_fwd rstd " + what),
               out=_within(out.check("out " + what), fx["out"], K["out"], "proj_fwd out " + what, bf))
    dxn, dW, db = Guarded((M, Ccat), dt, dev), Guarded((C, Ccat), F32, dev, fx["dW0"]), Guarded((C,), F32, dev, torch.zeros(C, dtype=F64))
    mean32, rstd32 = fx["mean"].float(), fx["rstd"].v.float()
    assert ep.proj_bwd(put(fx["d"], dt, dev), cat, mean32.to(dev), rstd32.to(dev), f("gamma"), f("beta"), f("W"), dxn.t, dW.t, db.t) == 0
    v, A, k = _prod_terms(RE(fx["d"]), fx["xn"])
    rec["dW"] = _sum_within(dW.check("dW " + what), fx["dW0"], v, A, k, M, "proj_bwd dW " + what)
    dxn.check("dxn " + what)
    assert_equal(db.check("db " + what), fx["d"].sum(0), "proj_bwd db " + what)
    record(f"proj/{M}x{Ccat}/C{C}/{dtn}", **rec)
