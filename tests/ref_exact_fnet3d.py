"""Exact-arithmetic fixtures for the conv3d / bn3d kernel family (viscy_amd/csrc/conv3d.hip).

Operands are small integers (activations, gradients, weights in {-2 .. 2}; biases and the old values of an accumulating output in
{-8 .. 8}), all exact in bf16 and fp32.  Every product is an integer, and while ``sum_k |a_k| |w_k| < 2^24`` every partial sum in
any order, in any split, inside or outside the matrix cores, is an integer below 2^24 and therefore exact in fp32.  So an fp32
output equals the float64 statement bit for bit and a bf16 output equals the statement rounded once to bf16: no tolerance.

This module holds the integer generators, the float64 statements, the precondition check, the mismatch report, the case tables
and the case runners.  A runner takes the op namespace as an argument, so the same table runs on ``viscy_amd.ops`` (GPU) and on
the fp32 torch statements of ``tests/ref_ops_fnet3d.py`` (CPU).  No GPU is needed to import it."""

from __future__ import annotations

import functools

import torch
import torch.nn.functional as F
from torch import Tensor

LIMIT = 2 ** 24   # integers below it are exact in fp32
SENT = 77.0       # what the columns outside an operand / output slice hold (exact in bf16)
U32 = 2.0 ** -24  # unit round-off of fp32
U16 = 2.0 ** -8   # unit round-off of bf16 (8 significant bits)
SLACK = 1.0 + 2.0 ** -20  # second-order terms of a derived bound and the float64 statement's own rounding


# ------------------------------------------------------------------------------------------------ operands
def ints(shape, lo: int, hi: int, seed: int) -> Tensor:
    """seeded integers in [lo, hi] as a float64 CPU tensor"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def choice(values, shape, seed: int) -> Tensor:
    v = torch.tensor(values, dtype=torch.float64)
    return v[ints(shape, 0, len(values) - 1, seed).long()]


def embed(vals: Tensor, coff: int, ld: int, dtype: torch.dtype, device, sentinel: float = SENT) -> Tensor:
    """[M, ld] buffer in ``dtype`` on ``device`` holding ``vals`` in columns [coff, coff + C) and the sentinel elsewhere"""
    M, C = vals.shape
    assert coff >= 0 and coff + C <= ld
    buf = torch.full((M, ld), sentinel, dtype=dtype)
    buf[:, coff:coff + C] = vals.to(dtype)
    return buf.to(device)


def rows_to_grid(m: Tensor, grid) -> Tensor:
    """[B*D*H*W, C] -> [B, C, D, H, W]"""
    B, D, H, W = grid
    return m.reshape(B, D, H, W, m.shape[1]).movedim(4, 1)


def grid_to_rows(x: Tensor) -> Tensor:
    """[B, C, D, H, W] -> [B*D*H*W, C]"""
    return x.movedim(1, 4).reshape(-1, x.shape[1])


def assert_exact_precondition(k_total: int, amax: float, wmax: float, extra: float = 0.0, what: str = "") -> None:
    """every partial sum of ``k_total`` products (+ ``extra``: bias, old value) stays an integer below 2^24"""
    bound = float(k_total) * float(amax) * float(wmax) + float(extra)
    assert bound < LIMIT, f"{what}: {k_total} x {amax} x {wmax} + {extra} = {bound:.0f} >= 2^24: fp32 is not exact here"


def _amax(t: Tensor) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------------ float64 statements
def conv_ref(role: str, a: Tensor, w: Tensor, grid, stride: int = 1, bias: Tensor | None = None, old: Tensor | None = None) -> Tensor:
    """float64 statement of ``ops.c3_conv`` for a weight role; ``a`` is [M, cin] on ``grid``, the result [Mo, cout]"""
    assert a.dtype == torch.float64 and w.dtype == torch.float64
    x = rows_to_grid(a, grid)
    if role == "conv":                       # Conv3d weight [cout, cin]
        y = F.conv3d(x, w, stride=stride, padding=1)
    elif role == "convT_dgrad":              # ConvTranspose3d weight [cin_T, cout_T]: its adjoint is a stride-2 convolution
        y = F.conv3d(x, w, stride=2, padding=1)
    elif role == "conv_dgrad_s1":            # adjoint of a stride-1 convolution
        y = F.conv_transpose3d(x, w, stride=1, padding=1)
    elif role in ("convT", "conv_dgrad_s2"):  # k 3, stride 2, padding 1, output_padding 1
        y = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    else:
        raise ValueError(role)
    y = grid_to_rows(y)
    if bias is not None:
        y = y + bias[None, :]
    if old is not None:
        y = y + old
    return y.contiguous()


def wgrad_ref(P: Tensor, Q: Tensor, gridP, stride: int, old: Tensor | None = None) -> Tensor:
    """float64 statement of ``ops.c3_wgrad``: dW[r, c, k] = sum_m P[m, r] Q[m * stride + k - 1, c]  (+ old)"""
    B, D, H, W = gridP
    R, Cq = P.shape[1], Q.shape[1]
    gP = rows_to_grid(P, gridP).contiguous()
    gQ = rows_to_grid(Q, (B, D * stride, H * stride, W * stride)).contiguous()
    dW = torch.nn.grad.conv3d_weight(gQ, (R, Cq, 3, 3, 3), gP, stride=stride, padding=1)
    return dW if old is None else dW + old


def colsum_ref(x: Tensor, old: Tensor | None = None) -> Tensor:
    s = x.sum(0)
    return s if old is None else s + old


def to_cl_ref(x: Tensor) -> Tensor:
    return grid_to_rows(x).contiguous()


def from_cl_ref(y: Tensor, B: int, spatial) -> Tensor:
    return rows_to_grid(y, (B, *spatial)).contiguous()


# ------------------------------------------------------------------------------------------------ comparison
def mismatch_report(got: Tensor, ref: Tensor, grid=None, parity: bool = False, what: str = "", limit: int = 8):
    """(count, text): the elements of ``got`` that differ from ``ref`` ([rows, channels] when ``grid`` = (B, D, H, W) of the rows),
    the first of them decoded to (b, z, y, x, channel), for a transposed convolution with the output parity class, and how they
    spread over rows, 64-row tiles and columns"""
    g, r = got.detach().cpu(), ref.detach().cpu()
    if g.shape != r.shape:
        return max(g.numel(), r.numel(), 1), f"{what}: shape {tuple(g.shape)} against {tuple(r.shape)}"
    bad = ~(g.double() == r.double())  # NaN counts
    n = int(bad.sum())
    if n == 0:
        return 0, f"{what}: equal"
    idx = bad.reshape(-1).nonzero().reshape(-1)
    ncol = g.shape[-1] if g.ndim > 1 else 1
    rows, cols = idx // ncol, idx % ncol
    lines = [f"{what}: {n} of {g.numel()} elements differ; {rows.unique().numel()} rows, {cols.unique().numel()} columns; "
             f"rows {int(rows.min())} .. {int(rows.max())}, columns {int(cols.min())} .. {int(cols.max())}; "
             f"row % 64 in {sorted(set((rows % 64).tolist()))[:16]}, column % 64 in {sorted(set((cols % 64).tolist()))[:16]}"]
    if grid is not None and g.ndim == 2 and g.shape[0] == grid[0] * grid[1] * grid[2] * grid[3]:
        B, D, H, W = grid
        x, y, z, b = rows % W, (rows // W) % H, (rows // (W * H)) % D, rows // (W * H * D)
        if parity:
            cls = ((z & 1) << 2) | ((y & 1) << 1) | (x & 1)
            lines.append("parity classes (pz py px): " + str({int(c): int((cls == c).sum()) for c in cls.unique()}))
        face = ((z == 0) | (z == D - 1) | (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1))
        lines.append(f"{int(face.sum())} of them on a face of the volume")
        for i in range(min(limit, n)):
            k = int(idx[i])
            lines.append(f"  (b {int(b[i])}, z {int(z[i])}, y {int(y[i])}, x {int(x[i])}, ch {int(cols[i])}): "
                         f"got {float(g.reshape(-1)[k])!r}, expected {float(r.reshape(-1)[k])!r}")
    else:
        for i in range(min(limit, n)):
            k = int(idx[i])
            lines.append(f"  flat {k} (row {int(rows[i])}, col {int(cols[i])}): got {float(g.reshape(-1)[k])!r}, "
                         f"expected {float(r.reshape(-1)[k])!r}")
    return n, "\n".join(lines)


def expect(ref64: Tensor, dtype: torch.dtype) -> Tensor:
    """the float64 statement in the storage type: exact for fp32 (asserted), rounded once to nearest-even for bf16"""
    e = ref64.to(dtype)
    if dtype == torch.float32:
        assert torch.equal(e.double(), ref64), "the float64 statement is not representable in fp32: fixture out of budget"
    return e


def assert_bit_equal(got: Tensor, ref64: Tensor, what: str, grid=None, parity: bool = False) -> None:
    ref = expect(ref64, got.dtype)
    g = got.detach().cpu()
    if not torch.equal(g, ref):
        raise AssertionError(mismatch_report(g, ref, grid, parity, what)[1])


def assert_sentinel(buf: Tensor, coff: int, C: int, what: str) -> None:
    """the columns outside [coff, coff + C) still hold the sentinel"""
    b = buf.detach().cpu()
    for part, lo in ((b[:, :coff], 0), (b[:, coff + C:], coff + C)):
        if part.numel():
            assert torch.equal(part, torch.full_like(part, SENT)), \
                f"{what}: columns outside the slice (from {lo}) were written: " + mismatch_report(part, torch.full_like(part, SENT))[1]


def assert_stats(stats: Tensor, stored: Tensor, what: str) -> None:
    """BatchNorm partials of a convolution epilogue, folded here in float64.
    Column 0, the sum of the stored values: a 64-row partial of stored integers is exact in fp32 while 64 max|stored| < 2^24, and
    the float64 fold of integers is exact, so it equals the float64 column sum bit for bit.
    Column 1, the sum of squares: per partial, 64 non-negative fp32 terms, each square rounded once (relative error <= u) and
    added with at most 63 roundings: for a sum of non-negative terms the relative error is at most (1 + u)^64 - 1 <= 65 u,
    u = 2^-24, and a float64 fold of non-negative partials keeps a relative bound.  Asserted per column: |s2 - ref| <= 65 u ref."""
    z = stored.detach().double().cpu()
    assert 64 * _amax(z) < LIMIT, f"{what}: stored values too large for exact 64-row partials"
    s = stats.detach().double().sum(0).cpu()
    n, msg = mismatch_report(s[0], z.sum(0), what=what + " stats[0] (sum z)")
    assert torch.equal(s[0], z.sum(0)), msg
    ref2 = (z * z).sum(0)
    err = (s[1] - ref2).abs()
    assert bool((err <= 65 * U32 * ref2).all()), f"{what} stats[1] (sum z^2): worst {float((err / ref2.clamp_min(1e-300)).max()):.3e} > 65 * 2^-24"


# ------------------------------------------------------------------------------------------------ convolution cases
def conv_case(name, kind, grid, cin, cout, a_layouts=None, ldc=None, ccoff=0, out_f32=False, fwd_acc=False,
              dy_ld=None, dy_coff=0, dx_ld=None, dx_coff=0, dx_acc=False):
    """kind: "s1" / "s2" (Conv3d, stride 1 / 2) or "T" (ConvTranspose3d k 3 s 2); ``grid`` = (B, D, H, W) of the forward input.
    a_layouts: (acoff, lda) of the forward operand, one launch each (the weight gradient reads the last);
    [ldc, ccoff]: the forward output slice; dy_*: the upstream gradient slice; dx_*: the data-gradient output slice"""
    return dict(name=name, kind=kind, grid=tuple(grid), cin=cin, cout=cout, a_layouts=list(a_layouts or [(0, cin)]),
                ldc=ldc or cout, ccoff=ccoff, out_f32=out_f32, fwd_acc=fwd_acc, dy_ld=dy_ld or cout, dy_coff=dy_coff,
                dx_ld=dx_ld or cin, dx_coff=dx_coff, dx_acc=dx_acc)


def layer_cases(patch=(32, 64, 64), b_wide=3, b_deep=24, b_thin=24, mult=32, depth=4):
    """every distinct convolution launch of Unet3d(1, 1, depth, mult) on ``patch`` with the operand layout of
    viscy_amd/engine_unet3d.py: forward, the matching data gradient and the weight gradient of each"""
    dims = [mult << l for l in range(depth + 1)]
    D, H, W = patch
    lev = lambda B, l: (B, D >> l, H >> l, W >> l)
    bat = lambda l: b_wide if dims[l] <= 128 else b_deep
    c0 = dims[0]
    cases = [conv_case(f"inconv_1_{c0}", "s1", lev(b_thin, 0), 1, c0)]
    for l in range(depth):
        c = dims[l]
        cases.append(conv_case(f"L{l}_block_{c}_{c}", "s1", lev(bat(l), l), c, c))
        # the downsampling convolution reads the skip half of the [M, 2c] concat buffer; its data gradient is added into the
        # skip half of the concat gradient
        cases.append(conv_case(f"L{l}_down_{c}_{2 * c}", "s2", lev(bat(l), l), c, 2 * c, a_layouts=[(c, 2 * c)],
                               dx_ld=2 * c, dx_coff=c, dx_acc=True))
        # the transposed convolution writes the first half of the concat buffer; its gradient is the first half of the
        # decoder block's input gradient
        cases.append(conv_case(f"L{l}_up_{2 * c}_{c}", "T", lev(bat(l), l + 1), 2 * c, c, ldc=2 * c, ccoff=0, dy_ld=2 * c))
        cases.append(conv_case(f"L{l}_decoder_{2 * c}_{c}", "s1", lev(bat(l), l), 2 * c, c))
    cb = dims[depth]
    cases.append(conv_case(f"bottleneck_{cb}_{cb}", "s1", lev(b_deep, depth), cb, cb))
    cases.append(conv_case(f"outconv_{c0}_1", "s1", lev(b_thin, 0), c0, 1, out_f32=True))
    return cases


EDGE_CIN = (1, 3, 8, 12, 40, 72)
EDGE_COUT = (1, 33, 65, 100, 130)
EDGE_GRIDS = (("s1", (1, 6, 10, 14)), ("s1", (3, 5, 7, 9)), ("s2", (2, 6, 10, 12)), ("T", (2, 3, 5, 6)))


def _edge(kind, grid, cin, cout):
    """operand at column 0 / 8 / 16 of a buffer whose row stride is a multiple of 8 (the vector gather when cin allows it) and at
    column 3 of an odd-stride buffer (the element-wise gather); output in the middle of a wider buffer; accumulating data gradient"""
    lda = (cin + 16 + 7) // 8 * 8 + 8
    name = f"{kind}_{'x'.join(map(str, grid))}_cin{cin}_cout{cout}"
    return conv_case(name, kind, grid, cin, cout, a_layouts=[(0, lda), (8, lda), (16, lda), (3, cin + 6)], ldc=cout + 9, ccoff=5,
                     fwd_acc=True, dy_ld=cout + 8, dy_coff=4, dx_ld=cin + 5, dx_coff=2, dx_acc=True)


def edge_cases():
    cases = [_edge(k, g, ci, co) for k, g in EDGE_GRIDS for ci in EDGE_CIN for co in EDGE_COUT]
    # one voxel: stride 1 on (1, 1, 1, 1); stride 2 from (1, 2, 2, 2) to one voxel; transposed from one voxel to 8
    cases += [_edge("s1", (1, 1, 1, 1), 8, 33), _edge("s2", (1, 2, 2, 2), 8, 33), _edge("T", (1, 1, 1, 1), 8, 33)]
    return cases


def _geometry(case):
    B, D, H, W = case["grid"]
    kind = case["kind"]
    if kind == "s1":
        return dict(role="conv", stride=1, tr=False, ogrid=(B, D, H, W), role_d="conv_dgrad_s1", st_d=1, tr_d=False, taps=27)
    if kind == "s2":
        return dict(role="conv", stride=2, tr=False, ogrid=(B, D // 2, H // 2, W // 2), role_d="conv_dgrad_s2", st_d=2, tr_d=True,
                    taps=27)
    return dict(role="convT", stride=2, tr=True, ogrid=(B, 2 * D, 2 * H, 2 * W), role_d="convT_dgrad", st_d=2, tr_d=False, taps=27)


def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 1000003


def _conv_fixture(case):
    """integer operands and the float64 statements of one case (shared by both dtypes)"""
    g = _geometry(case)
    B, D, H, W = case["grid"]
    M = B * D * H * W
    Mo = g["ogrid"][0] * g["ogrid"][1] * g["ogrid"][2] * g["ogrid"][3]
    cin, cout, s0 = case["cin"], case["cout"], _seed(case["name"])
    fx = dict(M=M, Mo=Mo, **g)
    fx["a"] = a = ints((M, cin), -2, 2, s0 + 1)
    fx["w"] = w = ints((cin, cout, 3, 3, 3) if case["kind"] == "T" else (cout, cin, 3, 3, 3), -2, 2, s0 + 2)
    fx["bias"] = bias = ints((cout,), -8, 8, s0 + 3)
    fx["old"] = old = ints((Mo, cout), -8, 8, s0 + 4) if case["fwd_acc"] else None
    fx["dy"] = dy = ints((Mo, cout), -2, 2, s0 + 5)
    fx["dx_old"] = dx_old = ints((M, cin), -8, 8, s0 + 6) if case["dx_acc"] else None
    fx["dW_old"] = dW_old = ints(w.shape, -8, 8, s0 + 7)
    fx["db_old"] = db_old = ints((cout,), -8, 8, s0 + 8)
    name = case["name"]
    assert_exact_precondition(g["taps"] * cin, _amax(a), _amax(w), _amax(bias) + (_amax(old) if old is not None else 0), name + " forward")
    assert_exact_precondition(g["taps"] * cout, _amax(dy), _amax(w), _amax(dx_old) if dx_old is not None else 0, name + " data gradient")
    assert_exact_precondition(max(M, Mo), _amax(dy), _amax(a), _amax(dW_old), name + " weight gradient")
    assert_exact_precondition(Mo, _amax(dy), 1, _amax(db_old), name + " bias gradient")
    fx["y"] = conv_ref(g["role"], a, w, case["grid"], g["stride"], bias)
    fx["y_acc"] = fx["y"] + old if old is not None else None
    fx["dx"] = conv_ref(g["role_d"], dy, w, g["ogrid"], g["st_d"], None, dx_old)
    if case["kind"] == "T":
        fx["dW"] = wgrad_ref(a, dy, case["grid"], 2, dW_old)
    else:
        fx["dW"] = wgrad_ref(dy, a, g["ogrid"], g["stride"], dW_old)
    fx["db"] = colsum_ref(dy, db_old)
    return fx


_latest: dict = {}


def conv_fixture(case):
    """the fixture of ``case``; the latest one is kept, so the two dtypes of a case compute the statements once"""
    key = (case["name"], case["grid"])
    if _latest.get("key") != key:
        _latest.clear()
        _latest.update(key=key, fx=_conv_fixture(case))
    return _latest["fx"]


def clear_fixtures() -> None:
    """drop the kept fixtures (gigabytes of float64 at the real shapes)"""
    _latest.clear()
    bn_fixture_cached.cache_clear()


def run_conv_case(ops, case, dt: torch.dtype, device) -> None:
    """forward (+ bias, statistics, every operand layout, accumulate), data gradient, weight gradient and bias gradient of one case
    through ``ops``; every result bit-equal to the float64 statement"""
    fx = conv_fixture(case)
    name, cin, cout = f"{case['name']}[{str(dt).split('.')[-1]}]", case["cin"], case["cout"]
    grid, ogrid, M, Mo = case["grid"], fx["ogrid"], fx["M"], fx["Mo"]
    odt = torch.float32 if case["out_f32"] else dt
    f32 = lambda t: t.float().to(device)
    w, bias = f32(fx["w"]), f32(fx["bias"])
    ldc, ccoff = case["ldc"], case["ccoff"]
    wp = ops.c3_prep(w, fx["role"], dt)
    first = None
    for acoff, lda in case["a_layouts"]:
        a = embed(fx["a"], acoff, lda, dt, device)
        out = torch.full((Mo, ldc), SENT, dtype=odt, device=device)
        stats = ops.c3_conv(a, acoff, cin, wp, bias, out, ccoff, cout, grid, fx["stride"], fx["tr"], False, True)
        what = f"{name} forward (acoff {acoff}, lda {lda})"
        assert_bit_equal(out[:, ccoff:ccoff + cout], fx["y"], what, ogrid, fx["tr"])
        assert_sentinel(out, ccoff, cout, what)
        assert_stats(stats, out[:, ccoff:ccoff + cout], what)
        if first is None:
            first = out
        else:
            assert torch.equal(out, first), what + ": differs from the first operand layout"
    if case["fwd_acc"]:
        out = embed(fx["old"], ccoff, ldc, odt, device)
        stats = ops.c3_conv(a, acoff, cin, wp, bias, out, ccoff, cout, grid, fx["stride"], fx["tr"], True, True)
        what = f"{name} forward, accumulate"
        assert_bit_equal(out[:, ccoff:ccoff + cout], fx["y_acc"], what, ogrid, fx["tr"])
        assert_sentinel(out, ccoff, cout, what)
        assert_stats(stats, out[:, ccoff:ccoff + cout], what)
    del out, first, stats
    # data gradient
    dy = embed(fx["dy"], case["dy_coff"], case["dy_ld"], dt, device)
    dxc, dxl = case["dx_coff"], case["dx_ld"]
    if case["dx_acc"]:
        dx = embed(fx["dx_old"], dxc, dxl, dt, device)
    else:
        dx = torch.full((M, dxl), SENT, dtype=dt, device=device)
    ops.c3_conv(dy, case["dy_coff"], cout, ops.c3_prep(w, fx["role_d"], dt), None, dx, dxc, cin, ogrid, fx["st_d"], fx["tr_d"],
                case["dx_acc"])
    what = f"{name} data gradient ({fx['role_d']})"
    assert_bit_equal(dx[:, dxc:dxc + cin], fx["dx"], what, grid, fx["tr_d"])
    assert_sentinel(dx, dxc, cin, what)
    del dx
    # weight gradient (accumulates onto integer old values) with the P / Q roles of the engine
    dW = f32(fx["dW_old"]).contiguous()
    if case["kind"] == "T":
        ops.c3_wgrad(a, acoff, cin, dy, case["dy_coff"], cout, dW, grid, 2)
    else:
        ops.c3_wgrad(dy, case["dy_coff"], cout, a, acoff, cin, dW, ogrid, fx["stride"])
    assert_bit_equal(dW.reshape(dW.shape[0], -1), fx["dW"].reshape(dW.shape[0], -1), f"{name} weight gradient (rows r, columns c * 27 + tap)")
    db = f32(fx["db_old"]).contiguous()
    ops.c3_colsum(dy, case["dy_coff"], cout, db)
    assert_bit_equal(db, fx["db"], f"{name} bias gradient")


# ------------------------------------------------------------------------------------------------ BatchNorm cases
BN_CASES = [(3 * 8 * 32 * 64 * 64, 32), (24 * 2 * 4 * 4, 512), (945, 1), (945, 33), (945, 100)]  # (M, C)


def bn_fixture(M: int, C: int):
    """dyadic table (scale, shift, rstd in powers of two, integer mean), integer z / dy: every product below is exact"""
    s0 = 7000 + C
    gamma, rstd = choice([0.5, 1.0, 2.0], (C,), s0 + 1), choice([0.5, 1.0, 2.0], (C,), s0 + 2)
    mean, beta = ints((C,), -3, 3, s0 + 3), ints((C,), -2, 2, s0 + 4)
    scale = gamma * rstd
    fx = dict(gamma=gamma, ss=torch.stack([scale, beta - mean * scale, mean, rstd]))
    fx["z"] = z = ints((M, C), -8, 8, s0 + 5)
    fx["dy"] = dy = ints((M, C), -2, 2, s0 + 6)
    fx["dg_old"], fx["db_old"] = ints((C,), -8, 8, s0 + 7), ints((C,), -8, 8, s0 + 8)
    pre = z * fx["ss"][0] + fx["ss"][1]
    fx["y"] = pre.clamp_min(0)
    g = dy * (pre > 0)
    xh = (z - mean) * rstd
    # g xhat is a multiple of 1/2; a group of the column reduction owns at most 2048 rows (M <= 2^22)
    assert_exact_precondition(2048, 2 * _amax(g * xh), 1, 0, "bn3d partial sums")
    fx["g"], fx["xh"] = g, xh
    fx["sg"], fx["sgx"] = g.sum(0), (g * xh).sum(0)
    return fx


@functools.lru_cache(maxsize=1)
def bn_fixture_cached(M: int, C: int):
    return bn_fixture(M, C)


def run_bn_case(ops, M: int, C: int, dt: torch.dtype, device) -> None:
    fx = bn_fixture_cached(M, C)
    name = f"bn3d M {M} C {C} [{str(dt).split('.')[-1]}]"
    f32 = lambda t: t.float().to(device).contiguous()
    ss, gamma = f32(fx["ss"]), f32(fx["gamma"])
    z = fx["z"].to(dt).to(device)
    # apply + ReLU into the second half of a [M, 2C] buffer (the encoder block's slot of the concat buffer)
    dst = torch.full((M, 2 * C), SENT, dtype=dt, device=device)
    ops.bn3d_apply_relu(z, ss, dst, C)
    assert_bit_equal(dst[:, C:], fx["y"], name + " apply_relu")
    assert_sentinel(dst, C, C, name + " apply_relu")
    del dst
    dy = embed(fx["dy"], C, 2 * C, dt, device)
    for training in (False, True):
        dg, db = f32(fx["dg_old"]), f32(fx["db_old"])
        dz = ops.bn3d_bwd(dy, C, z, ss, gamma, dg, db, training)
        assert_bit_equal(dg, fx["dg_old"] + fx["sgx"], name + " dgamma")
        assert_bit_equal(db, fx["db_old"] + fx["sg"], name + " dbeta")
        k = (fx["gamma"] * fx["ss"][3])[None, :]  # a power of two: scaling by it is exact
        if not training:
            assert_bit_equal(dz, k * fx["g"], name + " dz (eval)")
            continue
        # dz = k (g - c0 - xhat c1), c0 = sum g / M, c1 = sum g xhat / M.  In fp32: c0, c1 rounded once from double (e1, e2),
        # t = fl(g - c0) (e3), p = fl(xhat c1) (e4), r = fl(t - p) (e5), every |e| <= u = 2^-24 (a fused multiply-add drops one).
        # |r - exact| <= u (|c0| + |g - c0| + 2 |xhat c1| + |g - c0 - xhat c1|) <= 3 u (|g| + |c0| + |xhat c1|) to first order;
        # SLACK covers the second-order terms, the double rounding of c0 / c1 and the float64 statement's own rounding.
        c0, c1 = (fx["sg"] / M)[None, :], (fx["sgx"] / M)[None, :]
        ref = k * (fx["g"] - c0 - fx["xh"] * c1)
        bound = k * 3 * U32 * SLACK * (fx["g"].abs() + c0.abs() + (fx["xh"] * c1).abs())
        if dt == torch.bfloat16:  # one rounding of the fp32 result to bf16: relative 2^-8 of the value rounded
            bound = bound + U16 * (ref.abs() + bound)
        err = (dz.detach().double().cpu() - ref).abs()
        worst = float((err - bound).max())
        assert worst <= 0, f"{name} dz (train): error exceeds the element-wise bound by {worst:.3e} at {int((err - bound).argmax())}"


def run_bn_finalize_case(ops, C: int, G: int, device, M: int = 4096) -> None:
    """integer partials whose mean and variance are dyadic (M a power of two); ss, running statistics, num_batches_tracked against
    float64, each to the roundings of its fp32 expression"""
    s0 = 9000 + C + G
    mean, var = ints((C,), -8, 8, s0 + 1) / 4, choice([0.25, 0.5, 1.0, 2.25, 4.0], (C,), s0 + 2)
    tot = torch.stack([mean * M, (var + mean * mean) * M])  # integers
    assert torch.equal(tot, tot.round()) and _amax(tot) + 50 * G < LIMIT
    parts = ints((G, 2, C), -50, 50, s0 + 3)
    parts[G - 1] = tot - parts[:G - 1].sum(0)
    gamma, beta = choice([0.5, 1.0, 2.0], (C,), s0 + 4), ints((C,), -2, 2, s0 + 5)
    rm, rv = ints((C,), -8, 8, s0 + 6) / 4, choice([0.5, 1.0, 2.0], (C,), s0 + 7)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))      # the kernel receives eps and momentum as fp32
    mom = float(torch.tensor(0.1, dtype=torch.float32))
    f32 = lambda t: t.float().to(device).contiguous()
    u = U32 * SLACK
    for training in (True, False):
        rm_d, rv_d = f32(rm), f32(rv)
        nbt = torch.full((), 5, dtype=torch.long, device=device)
        ss = ops.bn3d_finalize(f32(parts), M, C, f32(gamma), f32(beta), rm_d, rv_d, nbt, training, 1e-5, 0.1)
        ss = ss.double().cpu()
        m, v = (mean, var) if training else (rm, rv)
        rstd = 1.0 / torch.sqrt(v + eps)
        scale = gamma * rstd
        shift = beta - m * scale
        what = f"bn3d_finalize C {C} G {G} training {training}"
        assert torch.equal(ss[2], m), what + ": mean"
        # rstd: a float64 value rounded once to fp32; scale = gamma rstd with gamma a power of two: the same single rounding
        assert bool(((ss[3] - rstd).abs() <= u * rstd).all()), what + ": rstd"
        assert bool(((ss[0] - scale).abs() <= u * scale.abs()).all()), what + ": scale"
        # shift = beta - mean * scale: the rounding of scale times |mean|, the product's rounding, the difference's rounding
        assert bool(((ss[1] - shift).abs() <= u * (2 * (m * scale).abs() + shift.abs())).all()), what + ": shift"
        if training:
            rm_ref = (1.0 - mom) * rm + mom * mean
            rv_ref = (1.0 - mom) * rv + mom * (var * M / (M - 1))
            # computed in double by the kernel and rounded once to fp32
            assert bool(((rm_d.double().cpu() - rm_ref).abs() <= u * rm_ref.abs()).all()), what + ": running_mean"
            assert bool(((rv_d.double().cpu() - rv_ref).abs() <= u * rv_ref.abs()).all()), what + ": running_var"
            assert int(nbt) == 6, what + ": num_batches_tracked"
        else:
            assert torch.equal(rm_d.double().cpu(), rm) and torch.equal(rv_d.double().cpu(), rv) and int(nbt) == 5, what


# ------------------------------------------------------------------------------------------------ layout cases
def run_layout_case(ops, C: int, dt: torch.dtype, device, B: int = 2, spatial=(3, 5, 7)) -> None:
    x = ints((B, C, *spatial), -8, 8, 500 + C)
    cl = ops.c3_to_cl(x.float().to(device), dt)
    assert cl.dtype == dt and tuple(cl.shape) == (B * spatial[0] * spatial[1] * spatial[2], C)
    assert_bit_equal(cl, to_cl_ref(x), f"c3_to_cl C {C}", (B, *spatial))
    back = ops.c3_from_cl(cl, B, spatial)
    assert back.dtype == torch.float32
    assert_bit_equal(back.reshape(B * C, -1), x.reshape(B * C, -1), f"c3_from_cl C {C} (round trip)")
    y = ints((B * spatial[0] * spatial[1] * spatial[2], C), -8, 8, 600 + C)
    assert_bit_equal(ops.c3_from_cl(y.to(dt).to(device), B, spatial).reshape(B * C, -1), from_cl_ref(y, B, spatial).reshape(B * C, -1),
                     f"c3_from_cl C {C}")
