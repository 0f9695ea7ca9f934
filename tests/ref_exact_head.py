"""Exact-arithmetic fixtures for the 2.5-D output head: the direct LDS-tiled 3x3x3 convolution (csrc/headconv.hip: forward in two
kernels, weight gradient, data gradient and its weight pre-pack), the head's pixel-shuffle + pad-pool permutations in their three
kernel tiers (csrc/spatial.hip) and the FCMAE voxel shuffle (csrc/spatial.hip, csrc/narrow.hip).

The method is that of tests/ref_exact_fnet3d.py and tests/ref_exact_gemm.py, whose helpers are imported: operands are small
integers, so every partial sum in any order, in any split over tiles, workgroups or atomics is an integer below 2^24 and fp32
arithmetic is exact.  An fp32 output equals the float64 statement bit for bit, a bf16 output equals the statement rounded once.

Convolution.  The forward's operands are in {-1, 0, 1} and its bias in {-8 .. 8}: max |U| <= 216 + 8 < 256, so every stored
value is an integer that bf16 holds exactly, and the InstanceNorm sums of a sample of at most 64 x 64 pixels stay below 2^24
(asserted on the statement: sum |c| <= sum c^2 < 2^24 per sample and channel).  Both ways the entry point forms these sums, the
atomics and the fixed-order pass (det_group_sum_kernel), ADD to ssum / ssq: they start from integer old values.  The two
gradients use {-2 .. 2} for dU, hin and the weights: |dW| <= 4 * B * H2 * W2 * 5 + 8, |dhin| <= 4 * 864.  dW / db start from
integer old values; U and dhin start as NaN (``nan_outputs``).

Shuffles.  Inputs are integers in {-8 .. 8}: a value pooled over 2 x 2 is a multiple of 1/4 of magnitude at most 8, one pooled
over 4 x 4 a multiple of 1/16 with a numerator of at most 128, both exact in bf16 and in fp32 in any order.

The float64 statements go through F.conv3d / torch.nn.grad and F.pixel_shuffle + F.pad + F.avg_pool2d with autograd; the
plain-PyTorch ops of tests/ref_ops.py that the CPU file runs through the same tables are written tap by tap from the layout
comments of headconv.hip and share no code with them.

Each case carries a ``leg`` string with the dispatch arithmetic that makes it reach its kernel path; ``conv_plan``,
``shuffle_plan`` and ``voxel_passes`` restate that host arithmetic and tests/test_head_exact_cpu.py asserts the coverage
conditions from them.  A runner takes the op namespace, so the same tables run on ``viscy_amd.ops`` (GPU) and on the CPU
statements.  No GPU is needed to import this module."""

from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F
from torch import Tensor

from tests.ref_exact_fnet3d import LIMIT, assert_bit_equal, assert_exact_precondition, expect, ints
from tests.ref_exact_gemm import BF16, BOTH, F32, Flags, _amax, _seed, dtname

C3, CMID, ZO, D7, KW = 8, 32, 5, 7, 216   # the one shape the direct kernels are built for; KW = 27 * C3
ROWS_FWD_PERSIST, ROWS_STRIP_FWD, ROWS_STRIP_BWD = 32, 8, 16   # bits of the `head_rows` flag


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ dispatch arithmetic
def conv_plan(B: int, H2: int, W2: int) -> dict:
    """vsx_head_conv_fwd / vsx_head_conv_wgrad: tiles of 8 x 16 pixels (HF_TY x HF_TX, counted per sample by hc_tiles() of
    csrc/headconv.hip), x fastest, then y, then the sample.  The persistent forward
    gives workgroup g the tiles [g tiles_per_wg, (g + 1) tiles_per_wg); the weight gradient's workgroup g takes g, g + grid, .."""
    tiles_x, tiles_y = W2 // 16, H2 // 8
    per, ntiles = tiles_x * tiles_y, B * tiles_x * tiles_y
    tpw = cdiv(ntiles, 512)
    wgs = cdiv(ntiles, tpw)
    grid = min(ntiles, 512)
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, per_sample=per, ntiles=ntiles, tiles_per_wg=tpw, wgs=wgs,
                last=ntiles - (wgs - 1) * tpw, wgrad_grid=grid, wgrad_max=cdiv(ntiles, grid), wgrad_min=ntiles // grid)


def shuffle_plan(B: int, h: int, w: int, c3: int, D: int, dt, pool: bool, head_rows: int = 63, bwd: bool = False) -> dict:
    """vsx_head_shuffle_fwd / _bwd: column strips (bf16, pooled, C3 D = 56, 64 | w, bit 3 / 4 of head_rows), else LDS tiles
    (C3 D <= 64), else one thread per 16-byte vector (head_shuffle_launch of csrc/spatial.hip; rows_per_wg is its
    hs_rows_per_wg)"""
    bit = ROWS_STRIP_BWD if bwd else ROWS_STRIP_FWD
    if dt == BF16 and pool and (head_rows & bit) and c3 * D == 56 and w % 64 == 0:
        strips = B * (w // 64)
        rpw = max(8, min(h, h * strips // 512))
        return dict(tier="strip", strips=strips, rows_per_wg=rpw, ranges=cdiv(h, rpw))
    if c3 * D <= 64:
        ts = 8 if dt == BF16 else 4
        return dict(tier="tiled", ts=ts, tiles=(cdiv(h, ts), cdiv(w, ts)))
    return dict(tier="thread")


def voxel_passes(threads: int) -> int:
    """passes of the grid-stride loop: the grid is capped at 65536 workgroups of 256 threads"""
    return cdiv(threads, 256 * min(cdiv(threads, 256), 65536))


# ------------------------------------------------------------------------------------------------ helpers
@contextlib.contextmanager
def nan_outputs():
    """the ops allocate their outputs with torch.empty; inside this block such a buffer starts as NaN, so an element that no
    workgroup writes cannot pass by holding an old result"""
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def det_scope(ops, on: bool):
    """the calling thread's fixed-order sums (ops.det_scope); the CPU statements have one order only"""
    scope = getattr(ops, "det_scope", None)
    return scope() if (on and scope is not None) else contextlib.nullcontext()


def _to5(rows: Tensor, B, H, W, planes, ch) -> Tensor:
    """[B*H*W, planes*ch] -> [B, ch, planes, H, W]"""
    return rows.reshape(B, H, W, planes, ch).permute(0, 4, 3, 1, 2).contiguous()


def _from5(x: Tensor) -> Tensor:
    """[B, ch, planes, H, W] -> [B*H*W, planes*ch]"""
    B, ch, planes, H, W = x.shape
    return x.permute(0, 3, 4, 2, 1).reshape(B * H * W, planes * ch).contiguous()


def prepared(w_par: Tensor) -> Tensor:
    """Conv3d weight [n, c, kz, ky, kx] -> the prepared layout [n, ((dy*3 + dx)*3 + dz)*8 + c] of headconv.hip"""
    return w_par.permute(0, 3, 4, 2, 1).reshape(w_par.shape[0], -1).contiguous()


_FIX: dict = {}


def _kept(family: str, name: str) -> dict:
    """the fixture of the latest case of a family: its flag variants, dtypes and directions share the operands and statements"""
    cur = _FIX.get(family)
    if cur is None or cur["name"] != name:
        cur = _FIX[family] = dict(name=name)
    return cur


def clear_fixtures() -> None:
    _FIX.clear()


# ------------------------------------------------------------------------------------------------ direct convolution
def conv_cases():
    def case(name, B, H2, W2, why):
        p = conv_plan(B, H2, W2)
        leg = (f"{why}: {p['tiles_y']} x {p['tiles_x']} tiles per sample, ntiles = {p['ntiles']}; forward: tiles_per_wg = "
               f"cdiv({p['ntiles']}, 512) = {p['tiles_per_wg']}, {p['wgs']} workgroups, the last with {p['last']}; weight gradient: "
               f"grid = min(ntiles, 512) = {p['wgrad_grid']}, {p['wgrad_min']} .. {p['wgrad_max']} tiles per workgroup")
        return dict(name=name, B=B, H2=H2, W2=W2, leg=leg)
    return [
        case("one_tile_column_2x16x16", 2, 16, 16, "left and right border in the same tile, two tile rows"),
        case("interior_2x32x48", 2, 32, 48, "tiles with all eight neighbours"),
        case("persistent_37x32x112", 37, 32, 112, "tile ranges that cross tile rows and samples, a short last range, a second and "
             "third tile per weight-gradient workgroup"),
    ]


def conv_fixture(case) -> dict:
    fx = _kept("conv", case["name"])
    if "hin" in fx:
        return fx
    B, H2, W2, s0 = case["B"], case["H2"], case["W2"], _seed(case["name"])
    M = B * H2 * W2
    assert H2 <= 64 and W2 <= 128 and H2 * W2 <= 64 * 64, "the statistics budget is worked out for samples of at most 64 x 64 pixels"
    fx.update(M=M, grid=(B, 1, H2, W2))
    # forward: {-1, 0, 1}
    fx["hin"], fx["w_par"] = ints((M, D7 * C3), -1, 1, s0 + 1), ints((CMID, C3, 3, 3, 3), -1, 1, s0 + 2)
    fx["bias"] = ints((CMID,), -8, 8, s0 + 3)
    fx["ssum_old"], fx["ssq_old"] = ints((B, CMID), -8, 8, s0 + 4), ints((B, CMID), -8, 8, s0 + 5)
    # gradients: {-2 .. 2}
    fx["hin_g"], fx["dU"] = ints((M, D7 * C3), -2, 2, s0 + 6), ints((M, ZO * CMID), -2, 2, s0 + 7)
    fx["w_par_g"] = ints((CMID, C3, 3, 3, 3), -2, 2, s0 + 8)
    fx["dW_old"], fx["db_old"] = ints((CMID, KW), -8, 8, s0 + 9), ints((CMID,), -8, 8, s0 + 10)
    fx["dpar_old"] = ints((CMID, C3, 3, 3, 3), -8, 8, s0 + 11)
    for w in (fx["w_par"], fx["w_par_g"]):
        # zero handling: every (tap, channel) column acts on at least one output channel, so no tap can go unexercised
        assert bool((prepared(w) != 0).any(0).all()), case["name"] + ": a (tap, channel) column of the weights is zero for every output channel"
    return fx


def conv_statement(case, part: str) -> dict:
    """float64 through F.conv3d / torch.nn.grad on [B, c, planes, H, W]; computed once per case and part"""
    fx = conv_fixture(case)
    if part in fx:
        return fx[part]
    B, H2, W2, name = case["B"], case["H2"], case["W2"], case["name"]
    st = {}
    if part == "fwd":
        assert_exact_precondition(27 * C3, _amax(fx["hin"]), _amax(fx["w_par"]), _amax(fx["bias"]), name + " forward")
        U = _from5(F.conv3d(_to5(fx["hin"], B, H2, W2, D7, C3), fx["w_par"], fx["bias"], padding=(0, 1, 1)))
        assert _amax(U) <= 256 and torch.equal(U, U.round()), f"{name}: max |U| = {_amax(U)}: bf16 would round what the statistics sum"
        stored = U.to(BF16).double().view(B, H2 * W2 * ZO, CMID)
        sq = (stored * stored).sum(1)
        assert float(sq.max()) + 8 < LIMIT, f"{name}: sum c^2 per (sample, channel) reaches {float(sq.max()):.0f} >= 2^24"
        st.update(U=U, ssum=fx["ssum_old"] + stored.sum(1), ssq=fx["ssq_old"] + sq, umax=_amax(U), sqmax=float(sq.max()))
    elif part == "wgrad":
        assert_exact_precondition(fx["M"] * ZO, _amax(fx["dU"]), _amax(fx["hin_g"]), 8 + 8 + 8, name + " weight gradient (+ both old values)")
        g5 = _to5(fx["dU"], B, H2, W2, ZO, CMID)
        gw = torch.nn.grad.conv3d_weight(_to5(fx["hin_g"], B, H2, W2, D7, C3), (CMID, C3, 3, 3, 3), g5, padding=(0, 1, 1))
        st["dW"] = fx["dW_old"] + prepared(gw)
        st["db"] = fx["db_old"] + fx["dU"].view(-1, CMID).sum(0)
        # vsx_unprep_grad(tapmode = 1) adds the whole prepared buffer, old values included, into the parameter layout
        st["dpar"] = fx["dpar_old"] + fx["dW_old"].view(CMID, 3, 3, 3, C3).permute(0, 4, 3, 1, 2) + gw
    elif part == "dgrad":
        assert_exact_precondition(27 * CMID, _amax(fx["dU"]), _amax(fx["w_par_g"]), 0, name + " data gradient")
        g5 = _to5(fx["dU"], B, H2, W2, ZO, CMID)
        st["dhin"] = _from5(torch.nn.grad.conv3d_input((B, C3, D7, H2, W2), fx["w_par_g"], g5, padding=(0, 1, 1)))
        assert _amax(st["dhin"]) <= 4 * 864
    else:
        raise ValueError(part)
    fx[part] = st
    return st


CONV_PARTS = ("fwd", "wgrad", "dgrad")


def conv_fwd_variants(flags: Flags):
    """(flag setting, det scope): the persistent and the one-tile-per-workgroup kernel, each with atomics and with fixed-order sums"""
    cur = flags.get("head_rows")
    if cur is None:
        return [({}, False)]
    return [({"head_rows": hr}, det) for hr in (cur | ROWS_FWD_PERSIST, cur & ~ROWS_FWD_PERSIST) for det in (False, True)]


def run_conv_case(ops, case, part: str, device, flags: Flags = Flags()) -> None:
    fx, st = conv_fixture(case), conv_statement(case, part)
    B, H2, W2, grid = case["B"], case["H2"], case["W2"], conv_fixture(case)["grid"]
    dims = (B, H2, W2, C3, CMID, ZO)
    f32 = lambda t: t.float().to(device).contiguous()
    b16 = lambda t: t.to(BF16).to(device).contiguous()
    name = f"head_conv {case['name']}"
    if part == "fwd":
        hin, bias = b16(fx["hin"]), f32(fx["bias"])
        Wc, _ = ops.prep_weight(f32(fx["w_par"]), CMID, C3, 27, BF16, tapmode=1)
        assert_bit_equal(Wc, prepared(fx["w_par"]), name + " prepared weights (columns ((dy*3 + dx)*3 + dz)*8 + c)")
        first = None
        for setting, det in conv_fwd_variants(flags):
            what = f"{name} forward {setting or ''}{' det_scope' if det else ''}"
            ssum, ssq = f32(fx["ssum_old"]), f32(fx["ssq_old"])
            with flags.scoped(setting), det_scope(ops, det), nan_outputs():
                if flags.lib is not None:   # the setting is the one this variant is listed under
                    assert flags.get("head_rows") == setting["head_rows"] and (not det or flags.lib.vsx_det_active() == 1), what
                U = ops.head_conv_fwd(hin, Wc, bias, ssum, ssq, *dims)
            assert U.dtype == BF16
            assert_bit_equal(U, st["U"], what + " U (ch = plane * 32 + channel)", grid)
            assert_bit_equal(ssum, st["ssum"], what + " ssum (rows = samples)")
            assert_bit_equal(ssq, st["ssq"], what + " ssq (rows = samples)")
            got = (U.cpu(), ssum.cpu(), ssq.cpu())
            first = first or got
            assert all(torch.equal(a, b) for a, b in zip(got, first)), what + ": differs from the first setting"
    elif part == "wgrad":
        hin, dU = b16(fx["hin_g"]), b16(fx["dU"])
        dW, db, dpar = f32(fx["dW_old"]), f32(fx["db_old"]), f32(fx["dpar_old"])
        ops.head_conv_wgrad(hin, dU, dW, db, *dims)
        assert_bit_equal(dW, st["dW"], name + " dW (rows = output channel, columns ((dy*3 + dx)*3 + dz)*8 + c)")
        assert_bit_equal(db, st["db"], name + " db")
        ops.unprep_grad(dW, dpar, CMID, C3, 27, tapmode=1)
        assert_bit_equal(dpar.reshape(CMID, -1), st["dpar"].reshape(CMID, -1), name + " unprep_grad(tapmode = 1) (columns (c*3 + kz)*9 + ky*3 + kx)")
    else:
        dU, Wc = b16(fx["dU"]), b16(prepared(fx["w_par_g"]))
        with nan_outputs():
            dhin = ops.head_conv_dgrad(dU, ops.head_conv_dgrad_prep(Wc), *dims)
        assert dhin.dtype == BF16 and tuple(dhin.shape) == (fx["M"], D7 * C3)
        assert_bit_equal(dhin, st["dhin"], name + " dhin (ch = plane * 8 + channel)", grid)


# ------------------------------------------------------------------------------------------------ head shuffle
def shuffle_cases():
    """``sweep``: the pooled bf16 launches also run with bits 3 / 4 of head_rows cleared (the tiled tier on the same values)"""
    def case(name, B, h, w, c3, D, why, dts=BOTH, pools=(True, False), sweep=False):
        leg = why
        if sweep:
            p = shuffle_plan(B, h, w, c3, D, BF16, True)
            leg += (f": {p['strips']} strips, rows_per_wg = clamp({h} * {p['strips']} / 512, 8, {h}) = {p['rows_per_wg']}, "
                    f"{p['ranges']} row ranges per strip")
        return dict(name=name, B=B, h=h, w=w, c3=c3, D=D, dts=tuple(dts), pools=tuple(pools), sweep=sweep, leg=leg)
    return [
        case("tiled_2x9x11", 2, 9, 11, 8, 7, "LDS tiles: h, w multiples of neither 8 (bf16) nor 4 (fp32), two tiles each way"),
        case("strips_2x20x192", 2, 20, 192, 8, 7, "column strips, the first without and two with a left halo column", sweep=True),
        case("strips_rows9_72x64x64", 72, 64, 64, 8, 7, "column strips with row ranges longer than 8 that do not divide h", dts=(BF16,),
             pools=(True,), sweep=True),
        case("thread_per_element_2x5x7_d9", 2, 5, 7, 8, 9, "C3 D = 72 > 64: one thread per 16-byte vector"),
    ]


def _head_shuffle64(dec_nchw: Tensor, c3: int, D: int, pool: bool) -> Tensor:
    """F.pixel_shuffle + ConstantPad2d((1, 0, 1, 0)) + AvgPool2d(2, 1); channel c3 D + z of the reference becomes z C3 + c3"""
    x = F.pixel_shuffle(dec_nchw, 2)
    if pool:
        x = F.avg_pool2d(F.pad(x, (1, 0, 1, 0)), kernel_size=2, stride=1)
    B, _, H2, W2 = x.shape
    return x.view(B, c3, D, H2, W2).permute(0, 3, 4, 2, 1).reshape(B * H2 * W2, D * c3)


def shuffle_statement(case, direction: str, pool: bool) -> Tensor:
    fx = _kept("shuffle", case["name"])
    B, h, w, c3, D = case["B"], case["h"], case["w"], case["c3"], case["D"]
    s0 = _seed(case["name"])
    if "dec" not in fx:   # the operands are kept as int8: the large case holds 66 M values each way
        fx["dec"] = ints((B * h * w, 4 * c3 * D), -8, 8, s0 + 1).to(torch.int8)
        fx["dhin"] = ints((B * 4 * h * w, c3 * D), -8, 8, s0 + 2).to(torch.int8)
    key = (direction, pool)
    if key not in fx:
        if direction == "fwd":
            ref = _head_shuffle64(fx["dec"].double().view(B, h, w, -1).permute(0, 3, 1, 2), c3, D, pool).contiguous()
        else:
            with torch.enable_grad():
                xin = torch.zeros(B, 4 * c3 * D, h, w, dtype=torch.float64, requires_grad=True)
                (g,) = torch.autograd.grad(_head_shuffle64(xin, c3, D, pool), xin, fx["dhin"].double())
            ref = g.permute(0, 2, 3, 1).reshape(B * h * w, 4 * c3 * D).contiguous()
        assert _amax(ref) <= 8 and torch.equal(ref * 4, (ref * 4).round()) and torch.equal(expect(ref, BF16).double(), ref), case["name"]
        fx[key] = ref
    return fx[key]


def shuffle_variants(case, dt, pool: bool, flags: Flags):
    cur = flags.get("head_rows")
    if cur is None or not (case["sweep"] and dt == BF16 and pool):
        return [{}]
    both = ROWS_STRIP_FWD | ROWS_STRIP_BWD
    return [{"head_rows": cur | both}, {"head_rows": cur & ~both}]


def run_shuffle_case(ops, case, direction: str, device, flags: Flags = Flags()) -> None:
    """every dtype and pooling mode of one case in one direction, the strip cases on the strip and on the tiled tier"""
    B, h, w, c3, D = case["B"], case["h"], case["w"], case["c3"], case["D"]
    for pool in case["pools"]:
        ref = shuffle_statement(case, direction, pool)
        fx = _kept("shuffle", case["name"])
        for dt in case["dts"]:
            src = (fx["dec"] if direction == "fwd" else fx["dhin"]).to(dt).to(device)
            for setting in shuffle_variants(case, dt, pool, flags):
                what = f"head_shuffle_{direction} {case['name']}[{dtname(dt)}] pool {int(pool)} {setting or ''}"
                with flags.scoped(setting), nan_outputs():
                    got = (ops.head_shuffle_fwd if direction == "fwd" else ops.head_shuffle_bwd)(src, B, h, w, c3, D, pool)
                assert got.dtype == dt
                if direction == "fwd":
                    assert_bit_equal(got, ref, what + " (ch = plane * C3 + channel)", (B, 1, 2 * h, 2 * w))
                else:
                    assert_bit_equal(got, ref, what + " (ch = 4 (c3 D + z) + 2 dy + dx)", (B, 1, h, w))
                del got
            del src


# ------------------------------------------------------------------------------------------------ voxel shuffle
def voxel_cases():
    """``dirs``: the directions a case runs; ``narrow``: the backward is vsx_narrow_voxel_shuffle_bwd (fewer channels than one 16-byte
    vector: one thread per element).  The grid-stride loop of vsx_voxel_shuffle_bwd itself is not reached: it needs more than
    65536 * 256 vectors, 134 M bf16 values and as many fp32 gradients, whose float64 statement alone takes longer than a test may."""
    def case(name, B, h, w, cout, D, s, why, dts=BOTH, pools=(True, False), dirs=("fwd", "bwd"), narrow=False):
        cd = cout * D * s * s
        out = B * cout * D * h * s * w * s
        leg = (f"{why}: forward {out} threads, {voxel_passes(out)} pass(es); backward "
               + (f"{out} threads (one per element)" if narrow else f"{out // 8} / {out // 4} threads (bf16 / fp32 vectors)"))
        return dict(name=name, B=B, h=h, w=w, cout=cout, D=D, s=s, cd=cd, dts=tuple(dts), pools=tuple(pools), dirs=tuple(dirs),
                    narrow=narrow, leg=leg)
    return [
        case("s4_2x5x7", 2, 5, 7, 2, 3, 4, "odd h and w, 4 x 4 pooling"),
        case("s2_2x5x7", 2, 5, 7, 2, 3, 2, "odd h and w, 2 x 2 pooling"),
        case("stride_fwd_7x128x128_s4", 7, 128, 128, 2, 5, 4, "more outputs than 65536 * 256: the forward's stride loop runs twice",
             pools=(True,), dirs=("fwd",)),
        case("narrow_2x5x7_s2", 2, 5, 7, 1, 1, 2, "Cout D s^2 = 4 channels, half a 16-byte bf16 vector (the 2 x 2 pre-training head)", dirs=("bwd",),
             narrow=True),
        case("narrow_2x5x7_d3_s2", 2, 5, 7, 1, 3, 2, "Cout D s^2 = 12 channels, no multiple of a bf16 vector", dirs=("bwd",), narrow=True),
        case("narrow_stride_bwd_5x1024x1024_s2", 5, 1024, 1024, 1, 1, 2, "more elements than 65536 * 256: the narrow backward's stride loop runs twice",
             dts=(BF16,), pools=(True,), dirs=("bwd",), narrow=True),
    ]


def _voxel_shuffle64(feat: Tensor, B, h, w, cout, D, s, pool: bool) -> Tensor:
    """nn.PixelShuffle(s) + ConstantPad2d((s - 1, 0, s - 1, 0)) + AvgPool2d(s, 1), reshaped to (B, Cout, D, s h, s w)"""
    x = F.pixel_shuffle(feat.view(B, h, w, cout * D * s * s).permute(0, 3, 1, 2), s)
    if pool:
        x = F.avg_pool2d(F.pad(x, (s - 1, 0, s - 1, 0)), kernel_size=s, stride=1)
    return x.reshape(B, cout, D, s * h, s * w)


def voxel_statement(case, direction: str, pool: bool) -> Tensor:
    fx = _kept("voxel", case["name"])
    geo = tuple(case[k] for k in ("B", "h", "w", "cout", "D", "s"))
    B, h, w, cout, D, s = geo
    s0 = _seed(case["name"])
    if "feat" not in fx:
        fx["feat"] = ints((B * h * w, case["cd"]), -8, 8, s0 + 1).to(torch.int8)
        fx["dout"] = ints((B, cout, D, s * h, s * w), -8, 8, s0 + 2).to(torch.int8)
    key = (direction, pool)
    if key not in fx:
        if direction == "fwd":
            ref = _voxel_shuffle64(fx["feat"].double(), *geo, pool).contiguous()
        else:
            with torch.enable_grad():
                f = torch.zeros(B * h * w, case["cd"], dtype=torch.float64, requires_grad=True)
                (ref,) = torch.autograd.grad(_voxel_shuffle64(f, *geo, pool), f, fx["dout"].double())
        q = s * s
        assert _amax(ref) <= 8 and torch.equal(ref * q, (ref * q).round()) and torch.equal(expect(ref, BF16).double(), ref), case["name"]
        fx[key] = ref
    return fx[key]


def run_voxel_case(ops, case, direction: str, device) -> None:
    geo = tuple(case[k] for k in ("B", "h", "w", "cout", "D", "s"))
    B = geo[0]
    for pool in case["pools"]:
        ref = voxel_statement(case, direction, pool)
        fx = _kept("voxel", case["name"])
        for dt in case["dts"]:
            what = f"voxel_shuffle_{direction} {case['name']}[{dtname(dt)}] pool {int(pool)}"
            with nan_outputs():
                if direction == "fwd":
                    got = ops.voxel_shuffle_fwd(fx["feat"].to(dt).to(device), *geo, pool)
                    assert got.dtype == F32 and tuple(got.shape) == tuple(ref.shape)
                    rows = B * case["cout"] * case["D"] * case["h"] * case["s"]
                    assert_bit_equal(got.reshape(rows, -1), ref.reshape(rows, -1), what + " (rows = ((b Cout + co) D + z) H + Y, columns X)")
                else:
                    op = ops.narrow_voxel_shuffle_bwd if case["narrow"] else ops.voxel_shuffle_bwd
                    got = op(fx["dout"].float().to(device), *geo, pool, dt)
                    assert got.dtype == dt
                    assert_bit_equal(got, ref, what + " (ch = ((co D + z) s + dy) s + dx)", (B, 1, case["h"], case["w"]))
            del got
