"""Exact-arithmetic fixtures for the 2-D kernel families that carry the training step: the NT / TN GEMMs (csrc/gemm.hip,
csrc/gemm_nt2.hip) and the depthwise 7x7 convolution (csrc/dwconv.hip, csrc/dwconv_mfma.hip).

The method is that of tests/ref_exact_fnet3d.py, whose generic helpers are imported: operands are small integers (activations,
gradients, weights in {-2 .. 2}, {-1, 0, 1} where a bound needs it; biases, residuals and the old contents of accumulating
outputs in {-8 .. 8}), so every partial sum in any order, in any split, on or off the matrix cores is an integer below 2^24.  An
fp32 output equals the float64 statement bit for bit and a bf16 output equals the statement rounded once to bf16.  One product
dropped from a K loop, one pixel row lost at a split boundary, one row of per-sample statistics credited to the neighbouring
sample or one depthwise tap wrong at one border moves an integer by at least 1 and fails, at any size.

Where an epilogue reduces the stored output (EPI_DZ, EPI_BIAS_STATS, the weight gradient with GRN statistics) the fixture also
asserts max |c| <= 256 on the statement: the bf16 value and the fp32 value it was rounded from are then the same integer, and the
check does not depend on which of the two the kernel sums.  The GRN prologue uses s in {0.5, 1, 2} and integer beta: operands are
half-integers, products multiples of 1/2, the budget 2^23.

Every operand sits inside a wider buffer whose other columns hold ``SENT``; NT outputs start as NaN inside their slice and
``SENT`` outside; TN outputs and every reduction target start from integer old values.

Each GEMM case names the kernel family (``vsx_last_kernel``) that the shipped dispatch sends it to, for each dtype; the runner
compares after every launch, so a case whose dispatch has moved fails instead of reporting a coverage it no longer gives.  The
instantiation below the family is not observable through the ABI: the ``leg`` string of a case records it together with the
dispatch condition that selects it (plan_nt / nt_fast_ok / vsx_gemm_nt2_ok / pick_bn / plan_tn of csrc/gemm.hip); the runner also asks
vsx_gemm_plan for the same parameters and flags and compares its family with the listed one.

A runner takes the op namespace as an argument, so the same tables run on ``viscy_amd.ops`` (GPU) and on the plain-PyTorch
statements of tests/ref_ops.py (CPU).  No GPU is needed to import this module."""

from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F
from torch import Tensor

from tests import ref_ops as R
from tests.ref_exact_fnet3d import LIMIT, SENT, assert_bit_equal, assert_exact_precondition, assert_sentinel, choice, embed, ints

F32, BF16 = torch.float32, torch.bfloat16
BOTH = (F32, BF16)
NT2, NT_FAST, NT_GEN, TN_FAST, TN_GEN = "gemm_nt2", "gemm_nt_fast", "gemm_nt_generic", "gemm_tn_fast", "gemm_tn_generic"
PAD = 8  # column offset of every operand / output slice inside its buffer (16-byte vectors: a multiple of 8 elements)


def dtname(dt) -> str:
    return "bf16" if dt == BF16 else "fp32"


def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 1000003


def _amax(t: Tensor) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------------ flags and dispatch
class Flags:
    """the tuning flags and the dispatch record of the library under test; the CPU reference (``lib`` None) has neither"""

    def __init__(self, lib=None):
        self.lib = lib

    @contextlib.contextmanager
    def scoped(self, settings):
        if self.lib is None or not settings:
            yield
            return
        saved = {n: self.lib.vsx_get_flag(n.encode()) for n in settings}
        try:
            for n, v in settings.items():
                assert self.lib.vsx_set_flag(n.encode(), int(v)) == 0, n
            yield
        finally:
            for n, v in saved.items():
                self.lib.vsx_set_flag(n.encode(), v)

    def get(self, name: str):
        return None if self.lib is None else int(self.lib.vsx_get_flag(name.encode()))

    def variants(self, sweep):
        """the flag settings of a sweep; one empty setting where there are no flags to set"""
        return list(sweep) if self.lib is not None else [{}]

    @staticmethod
    def plan_of(ops, kind, *args, **kw):
        """what ``ops.gemm`` with these arguments would launch (one host call, no launch)"""
        from viscy_amd._lib import VsxGemmPlan

        plan = VsxGemmPlan()
        ops.gemm(kind, *args, plan=plan, **kw)
        return plan

    def check_family(self, want: str, what: str, plan=None) -> None:
        """``plan``: what vsx_gemm_plan answers for the parameters and flags of the launch just made"""
        if self.lib is None:
            return
        got = self.lib.vsx_last_kernel().decode()
        assert plan is None or plan.family.decode() == want, f"{what}: listed under {want}, planned as {plan.family.decode()}"
        assert got == want, (f"{what}: the case table lists this launch under {want}, the library dispatched it to {got}: the "
                             f"dispatch has moved and this case no longer covers the kernel it is listed for")


def family_of(case, dt) -> str:
    fam = case["fam"]
    return fam if isinstance(fam, str) else fam[dtname(dt)]


# ------------------------------------------------------------------------------------------------ float64 statements
def patch2_gather_ref(src: Tensor, B: int, gh: int, gw: int) -> Tensor:
    """[B * 2gh * 2gw, cs] -> [B * gh * gw, 4 cs]: column (2 ky + kx) cs + c of output pixel (y, x) is input pixel (2y + ky, 2x + kx)"""
    cs = src.shape[1]
    g = src.reshape(B, 2 * gh, 2 * gw, cs)
    return torch.cat([g[:, ky::2, kx::2, :] for ky in (0, 1) for kx in (0, 1)], dim=-1).reshape(B * gh * gw, 4 * cs)


def patch2_scatter_ref(out: Tensor, B: int, gh: int, gw: int) -> Tensor:
    """[B * gh * gw, 4 c] -> [B * 2gh * 2gw, c]: the transpose of patch2_gather_ref"""
    c = out.shape[1] // 4
    dst = torch.zeros(B, 2 * gh, 2 * gw, c, dtype=out.dtype)
    o = out.reshape(B, gh, gw, 4, c)
    for ky in (0, 1):
        for kx in (0, 1):
            dst[:, ky::2, kx::2, :] = o[:, :, :, 2 * ky + kx, :]
    return dst.reshape(B * 4 * gh * gw, c)


def conv3_gather_ref(src: Tensor, B: int, gh: int, gw: int) -> Tensor:
    """[B * gh * gw, cs] -> [B * gh * gw, 9 cs]: column (3 ky + kx) cs + c of pixel (y, x) is pixel (y + ky - 1, x + kx - 1), 0 outside"""
    cs = src.shape[1]
    g = src.reshape(B, gh, gw, cs)
    out = torch.zeros(B, gh, gw, 9, cs, dtype=src.dtype)
    for ky in range(3):
        for kx in range(3):
            y0, y1 = max(0, 1 - ky), min(gh, gh + 1 - ky)
            x0, x1 = max(0, 1 - kx), min(gw, gw + 1 - kx)
            out[:, y0:y1, x0:x1, 3 * ky + kx, :] = g[:, y0 + ky - 1:y1 + ky - 1, x0 + kx - 1:x1 + kx - 1, :]
    return out.reshape(B * gh * gw, 9 * cs)


def sample_of(M: int, hw: int) -> Tensor:
    return torch.arange(M) // (hw if hw > 0 else M)


def per_sample_sum(v: Tensor, hw: int) -> Tensor:
    M = v.shape[0]
    b = sample_of(M, hw)
    return torch.zeros(int(b.max()) + 1, v.shape[1], dtype=v.dtype).index_add_(0, b, v)


def dw_fwd_ref(x: Tensor, w: Tensor, bias: Tensor | None, B, H, W, C) -> Tensor:
    """y[b, y, x, c] = sum_t w[t, c] x[b, y + ky - 3, x + kx - 3, c] (+ bias), t = 7 ky + kx, zero outside the image"""
    xp = F.pad(x.reshape(B, H, W, C), (0, 0, 3, 3, 3, 3))
    y = torch.zeros(B, H, W, C, dtype=x.dtype)
    for ky in range(7):
        for kx in range(7):
            y += xp[:, ky:ky + H, kx:kx + W, :] * w[7 * ky + kx]
    if bias is not None:
        y = y + bias
    return y.reshape(B * H * W, C)


def dw_bwd_data_ref(dy: Tensor, w: Tensor, add: Tensor | None, B, H, W, C) -> Tensor:
    """the adjoint: the same sum with the taps mirrored (+ add)"""
    dx = dw_fwd_ref(dy, w.flip(0), None, B, H, W, C)
    return dx if add is None else dx + add


def dw_bwd_weight_ref(dy: Tensor, x: Tensor, B, H, W, C):
    xp = F.pad(x.reshape(B, H, W, C), (0, 0, 3, 3, 3, 3))
    g = dy.reshape(B, H, W, C)
    dw = torch.stack([(g * xp[:, ky:ky + H, kx:kx + W, :]).sum((0, 1, 2)) for ky in range(7) for kx in range(7)])
    return dw, dy.sum(0)


# ------------------------------------------------------------------------------------------------ NT cases
# epilogue variants: name -> (epi, bias, rscale)
EPIS = {
    "none": (R.EPI_NONE, False, False), "bias": (R.EPI_BIAS, True, False), "res": (R.EPI_BIAS_RES, True, False),
    "res_nobias": (R.EPI_BIAS_RES, False, False), "res_rscale": (R.EPI_BIAS_RES, True, True), "dz": (R.EPI_DZ, False, False),
    "stats": (R.EPI_BIAS_STATS, True, False), "gelu": (R.EPI_BIAS_GELU_SQ, True, False),
}
REDUCING = ("dz", "stats")
ALL6 = ("none", "bias", "res", "res_nobias", "dz", "stats", "gelu")   # what the generic kernel takes
LEAN = ("none", "bias", "res", "res_nobias", "dz", "gelu")            # gemm_nt_fast_kernel: no EPI_BIAS_STATS
LEAN_PLAIN = ("none", "bias", "res")                                  # with a tile that is not made of whole samples
GEN2 = ("none", "bias", "res_rscale", "dz", "gelu")


def nt(name, M, N, K, hw, epis, fam, leg, dts=BOTH, flags=({},), **kw):
    """one NT launch shape.  ``fam``: the kernel family, or {"fp32": .., "bf16": ..}; ``flags``: the flag settings it runs under, one
    launch series each ({} = as shipped).  kw: a_mode / c_mode (+ grid = (B, gh, gw), cs / c_cs), pro, bstride (per-sample
    weights), nz (z-batched A_CONV3 slabs, with c3)"""
    return dict(name=name, M=M, N=N, K=K, hw=hw, epis=tuple(epis), fam=fam, leg=leg, dts=tuple(dts), flags=tuple(flags),
                a_mode=kw.pop("a_mode", R.A_ROWS), c_mode=kw.pop("c_mode", R.A_ROWS), grid=kw.pop("grid", None), cs=kw.pop("cs", 0),
                c_cs=kw.pop("c_cs", 0), pro=kw.pop("pro", R.PRO_NONE), bstride=kw.pop("bstride", False), nz=kw.pop("nz", 1),
                c3=kw.pop("c3", 0), **kw)


def nt_cases():
    c = []
    # ---- generic tiles (N <= 64: gemm_nt_kernel<T, 128, 64 / 32 / 16>, BK = 32); ragged rows, tiles that span several samples
    gen = [(130, 8, 72, 100), (8, 16, 8, 4), (200, 24, 40, 100), (130, 32, 8, 4), (200, 40, 72, 4), (8, 64, 40, 4)]
    for M, N, K, hw in gen:
        bn = 16 if N <= 16 else (32 if N <= 32 else 64)
        c.append(nt(f"generic_{M}x{N}x{K}_hw{hw}", M, N, K, hw, ALL6, NT_GEN, f"N <= {bn}: gemm_nt_kernel<T, 128, {bn}, .., 32>"))
    c.append(nt("generic_grn_200x40x72_hw100", 200, 40, 72, 100, ("none", "res"), NT_GEN, "N <= 64, GRN prologue in lstore", pro=R.PRO_GRN))
    c.append(nt("generic_n72_lean_off", 200, 72, 40, 100, ALL6, NT_GEN, "N > 64 with nt_fast = 0: gemm_nt_kernel<T, 128, 128, 2, 2, 32>",
                flags=({"nt_fast": 0},)))
    # ---- generic BK = 128 leg: bf16, N > 64, K >= 256, fewer than 512 tiles, not taken by gemm_nt2 (shipped nt2 = 17 wants
    #      >= 256 tiles and K >= 768; M % 256 != 0 here in any case)
    c.append(nt("generic_bk128_200x96x264_hw100", 200, 96, 264, 100, ALL6, NT_GEN, "tiles < 512 && K >= 256: gemm_nt_kernel<T, 128, 128, 2, 2, 128>; K % 128 = 8",
                dts=(BF16,)))
    c.append(nt("generic_bk128_384x224x512_hw128", 384, 224, 512, 128, ALL6, NT_GEN,
                "gemm_nt_kernel<T, 128, 128, 2, 2, 128>, ragged last N tile (M % 256 != 0: gemm_nt2 cannot take it at any nt2)", dts=(BF16,)))
    # ---- gemm_nt_fast_kernel
    c.append(nt("lean_bk32_384x192x224_hw128", 384, 192, 224, 128, LEAN, NT_FAST,
                "K < 256, N > 64, K % 32 == 0: bf16 <32, 1> (nt_wide != 0: BK = 32, one LDS buffer), fp32 the default instantiation"))
    c.append(nt("lean_bk32_grn_384x192x224_hw128", 384, 192, 224, 128, ("none", "res", "res_rscale"), NT_FAST, "the same with PRO = true", pro=R.PRO_GRN))
    c.append(nt("lean_ktail_200x96x72_hw128", 200, 96, 72, 128, LEAN, NT_FAST, "K % 32 != 0, K > 32 (nt_fast bit 1): zero-filled last slab; ragged M"))
    c.append(nt("lean_ktail_384x128x200_hw64", 384, 128, 200, 64, LEAN, NT_FAST, "K tail with two samples per tile (split_tile)"))
    c.append(nt("lean_patch2_gather_3x8x8_cs32_n96", 192, 96, 128, 64, ("none", "bias"), NT_FAST, "a_mode = A_PATCH2, cs % 32 == 0",
                a_mode=R.A_PATCH2, grid=(3, 8, 8), cs=32))
    c.append(nt("generic_patch2_gather_2x6x5_cs16_n24", 60, 24, 64, 30, ("none", "bias"), NT_GEN, "A_PATCH2 with cs % 32 != 0 and N <= 64",
                a_mode=R.A_PATCH2, grid=(2, 6, 5), cs=16))
    c.append(nt("lean_patch2_scatter_3x8x8_ccs24", 192, 96, 72, 64, ("none", "bias"), NT_FAST, "c_mode = A_PATCH2 (+ a K tail)",
                c_mode=R.A_PATCH2, grid=(3, 8, 8), c_cs=24))
    c.append(nt("generic_patch2_scatter_2x6x5_ccs8", 60, 32, 40, 30, ("none", "bias"), NT_GEN, "c_mode = A_PATCH2, N <= 64",
                c_mode=R.A_PATCH2, grid=(2, 6, 5), c_cs=8))
    c.append(nt("lean_two_samples_per_tile_448x192x224_hw64", 448, 192, 224, 64, LEAN, NT_FAST,
                "hw = 64: split_tile, 7 samples: the last tile holds one sample and an empty pass"))
    c.append(nt("lean_two_samples_grn_448x192x224_hw64", 448, 192, 224, 64, ("none", "res"), NT_FAST, "hw = 64 with the GRN prologue (s row per tile row)",
                pro=R.PRO_GRN))
    c.append(nt("lean_per_sample_weights_512x96x64_hw128", 512, 96, 64, 128, ("none", "res", "res_rscale"), NT_FAST,
                "b_bstride != 0: plan_nt sends it to the lean kernel (hw % 128 == 0)", bstride=True))
    # BK = 64 instantiations: bf16, K % 64 == 0, K >= 256; 172 x 3 = 516 tiles, the fewest that pass the `tiles < 512` test of the
    # BK = 128 generic leg (gemm_nt2 as shipped does not take K < 768)
    c.append(nt("lean_bk64_22016x384x256_hw128", 172 * 128, 384, 256, 128, ("none", "res_rscale", "dz"), NT_FAST,
                "nt_wide = 1: <64, 1> (one LDS buffer); nt_wide = 2: <64, 2>", dts=(BF16,), flags=({"nt_wide": 1}, {"nt_wide": 2})))
    # ---- gemm_nt2 (bf16, M % 256 == 0, K % 32 == 0; nt2 = 3 makes it take every launch it supports).  pick_bn: N = 128 -> 128,
    #      448 -> 256 (two tiles, the last 192 wide), 384 -> 384, 896 -> 384 (three tiles, the last 128 wide)
    g2 = dict(dts=(BF16,), flags=({"nt2": 3},))
    c.append(nt("gen2_bn128_512x128x96_hw256", 512, 128, 96, 256, GEN2, NT2, "pick_bn = 128, one sample per tile", **g2))
    c.append(nt("gen2_bn384_ragged_256x896x96_hw128", 256, 896, 96, 128, GEN2, NT2, "pick_bn = 384, ragged last tile, two samples per tile", **g2))
    c.append(nt("gen2_bn384_512x384x96_hw64", 512, 384, 96, 64, GEN2, NT2, "pick_bn = 384, four samples per tile", **g2))
    c.append(nt("gen2_bn256_512x448x64_hw256", 512, 448, 64, 256, GEN2, NT2, "pick_bn = 256, ragged last tile", **g2))
    c.append(nt("gen2_grn_512x128x96_hw256", 512, 128, 96, 256, ("none", "res", "res_rscale"), NT2, "PRO_GRN: hw % 256 == 0", pro=R.PRO_GRN, **g2))
    c.append(nt("gen2_per_sample_weights_512x96x96_hw256", 512, 96, 96, 256, ("res", "res_rscale"), NT2, "b_bstride with hw = 256", bstride=True, **g2))
    # ---- the head convolution's form: A_CONV3 with nz = 5 z-batched slabs on a 6 x 5 grid (all four borders inside one tile)
    c.append(nt("conv3_z5_5x6x5_c8_n32", 150, 32, 216, 30, ("stats", "bias", "none"), NT_GEN, "a_mode = A_CONV3, nz = 5, N <= 32",
                a_mode=R.A_CONV3, grid=(5, 6, 5), cs=24, nz=5, c3=8))
    return c


_NT_FIX: dict = {}


def nt_fixture(case):
    """integer operands and the float64 accumulator of one case (shared by its dtypes, epilogues and flag settings; the latest
    case is kept)"""
    key = (case["name"], case["epis"])
    if _NT_FIX.get("key") == key:
        return _NT_FIX["fx"]
    M, N, K, hw, nz, s0 = case["M"], case["N"], case["K"], case["hw"], case["nz"], _seed(case["name"])
    reducing = any(e in REDUCING for e in case["epis"])
    v = 1 if (reducing and K > 96) else 2   # keeps max |c| <= 256 where the stored output is reduced (asserted below)
    nb = (M + hw - 1) // hw
    fx = dict(nb=nb, v=v)
    if case["a_mode"] == R.A_PATCH2:
        B, gh, gw = case["grid"]
        fx["a_src"] = ints((4 * M, case["cs"]), -v, v, s0 + 1)
        a = [patch2_gather_ref(fx["a_src"], B, gh, gw)]
    elif case["a_mode"] == R.A_CONV3:
        B, gh, gw = case["grid"]
        c3 = case["c3"]
        fx["a_src"] = ints((M, (nz + 2) * c3), -v, v, s0 + 1)
        a = [conv3_gather_ref(fx["a_src"][:, z * c3:(z + 3) * c3], B, gh, gw) for z in range(nz)]
    else:
        fx["a_src"] = ints((M, K), -v, v, s0 + 1)
        a = [fx["a_src"]]
    assert a[0].shape == (M, K)
    b = sample_of(M, hw)
    amax = v
    if case["pro"] == R.PRO_GRN:
        fx["s"], fx["beta"] = choice([0.5, 1.0, 2.0], (nb, K), s0 + 2), ints((K,), -2, 2, s0 + 3)
        a = [t * fx["s"][b] + fx["beta"][None, :] for t in a]
        amax = 2 * v + 2
        assert all(torch.equal(t * 2, (t * 2).round()) and _amax(t) <= amax for t in a)
    if case["bstride"]:
        fx["w"] = w = ints((nb, N, K), -v, v, s0 + 4)
        acc = [torch.cat([t[b == i] @ w[i].t() for i in range(nb)]) for t in a]
    else:
        fx["w"] = w = ints((N, K), -v, v, s0 + 4)
        acc = [t @ w.t() for t in a]
    fx["acc"] = torch.cat(acc, dim=1)   # [M, nz * N]
    fx["bias"], fx["res"] = ints((N,), -8, 8, s0 + 5), ints((M, N), -8, 8, s0 + 6)
    fx["aux"] = ints((M, N), -v, v, s0 + 7)
    fx["rscale"] = (torch.arange(nb) % 2).double() * 1.25
    fx["r0_old"], fx["r1_old"] = ints((nb, N), -8, 8, s0 + 8), ints((nb, N), -8, 8, s0 + 9)
    # (acc + bias) * 1.25 + res: a multiple of 1/4 (1/8 with the GRN prologue): 8 x the integer budget
    assert_exact_precondition(K, amax, v, 8 + 8, case["name"] + " accumulator")
    assert 8 * (K * amax * v + 16) < LIMIT, case["name"] + ": the rscale epilogue leaves the exact range"
    _NT_FIX.clear()
    _NT_FIX.update(key=key, fx=fx)
    return fx


def nt_statement(case, fx, epi_name):
    """float64: (c [M, nz N], red0, red1) of one epilogue variant"""
    epi, with_bias, with_rscale = EPIS[epi_name]
    M, N, hw, nz = case["M"], case["N"], case["hw"], case["nz"]
    c = fx["acc"].clone()
    if with_bias:
        c = c + fx["bias"].repeat(nz)[None, :]
    if epi == R.EPI_BIAS_RES:
        if with_rscale:
            c = c * fx["rscale"][sample_of(M, hw)][:, None]
        c = c + fx["res"]
    r0 = r1 = None
    if epi_name in REDUCING:
        assert _amax(c) <= 256, f"{case['name']} [{epi_name}]: max |c| = {_amax(c)} > 256: bf16 would round what the epilogue reduces"
        assert torch.equal(c, c.round())
        parts = [c[:, z * N:(z + 1) * N] for z in range(nz)]
        if epi == R.EPI_DZ:
            assert_exact_precondition(min(hw, M), 256, fx["v"], 8, case["name"] + " red0")
            r0 = fx["r0_old"] + sum(per_sample_sum(p * fx["aux"], hw) for p in parts)
            r1 = fx["r1_old"] + sum(per_sample_sum(p, hw) for p in parts)
        else:
            assert_exact_precondition(min(hw, M) * nz, 256, 256, 8, case["name"] + " red1")
            r0 = fx["r0_old"] + sum(per_sample_sum(p, hw) for p in parts)
            r1 = fx["r1_old"] + sum(per_sample_sum(p * p, hw) for p in parts)
    return c, r0, r1


def run_nt_case(ops, case, dt, device, flags: Flags = Flags()) -> None:
    """every epilogue variant of one case under each of its flag settings through ``ops``: output, sentinels and reductions
    bit-equal to the float64 statement, and the dispatched kernel family equal to the one the table names"""
    fx = nt_fixture(case)
    M, N, K, hw, nz = case["M"], case["N"], case["K"], case["hw"], case["nz"]
    nb = fx["nb"]
    f32 = lambda t: t.float().to(device).contiguous()
    if case["a_mode"] == R.A_ROWS:
        A, a_coff, lda = embed(fx["a_src"], PAD, K + 2 * PAD, dt, device), [PAD], K + 2 * PAD
    elif case["a_mode"] == R.A_PATCH2:
        A, a_coff, lda = embed(fx["a_src"], PAD, case["cs"] + 2 * PAD, dt, device), [PAD], case["cs"] + 2 * PAD
    else:
        wsrc = fx["a_src"].shape[1]
        A, a_coff, lda = embed(fx["a_src"], PAD, wsrc + 2 * PAD, dt, device), [PAD + z * case["c3"] for z in range(nz)], wsrc + 2 * PAD
    ldb = K + PAD
    Bw = embed(fx["w"].reshape(-1, K), 0, ldb, dt, device)
    res, aux = embed(fx["res"], 0, N + PAD, dt, device), embed(fx["aux"], 0, N + PAD, dt, device)
    scatter = case["c_mode"] == R.A_PATCH2
    cw = case["c_cs"] if scatter else nz * N   # width of the output slice
    crows = 4 * M if scatter else M
    ldc, c_coff = cw + 2 * PAD, [PAD + z * N for z in range(nz)]
    kw0 = dict(dtype=dt, a_mode=case["a_mode"], c_mode=case["c_mode"], cs=case["cs"], c_cs=case["c_cs"], pro=case["pro"], hw=hw)
    if case["grid"] is not None:
        kw0.update(gh=case["grid"][1], gw=case["grid"][2])
    if case["pro"] == R.PRO_GRN:
        kw0.update(grn_s=f32(fx["s"]), grn_b=f32(fx["beta"]))
    if case["bstride"]:
        kw0.update(b_bstride=N * ldb)

    def out_buffer():
        buf = torch.full((crows, ldc), SENT, dtype=dt)
        buf[:, PAD:PAD + cw] = float("nan")
        return buf.to(device)

    for setting in flags.variants(case["flags"]):
        with flags.scoped(setting):
            for epi_name in case["epis"]:
                epi, with_bias, with_rscale = EPIS[epi_name]
                c64, r0_64, r1_64 = nt_statement(case, fx, epi_name)
                what = f"{case['name']}[{dtname(dt)}] {epi_name} {setting or ''}"
                kw = dict(kw0, epi=epi)
                if with_bias:
                    kw.update(bias=f32(fx["bias"]))
                if epi == R.EPI_BIAS_RES:
                    kw.update(res=res, ldr=N + PAD)
                if with_rscale:
                    kw.update(rscale=f32(fx["rscale"]))
                C, C2 = out_buffer(), None
                r0, r1 = f32(fx["r0_old"]), f32(fx["r1_old"])
                if epi == R.EPI_DZ:
                    kw.update(aux=aux, ldx=N + PAD, red0=r0, red1=r1)
                elif epi == R.EPI_BIAS_STATS:
                    kw.update(red0=r0, red1=r1)
                elif epi == R.EPI_BIAS_GELU_SQ:
                    C2 = out_buffer()
                    kw.update(red0=r0, C2=C2)
                args = (A, Bw, C, M, N, K, lda, ldb, ldc)
                if nz > 1:
                    ops.gemm_z("nt", *args, nz=nz, a_coff=a_coff, b_off=[0] * nz, c_coff=c_coff, **kw)
                else:
                    ops.gemm("nt", *args, a_coff=a_coff, c_coff=c_coff, **kw)
                plan = None if flags.lib is None else flags.plan_of(ops, "nt", *args, nz=min(nz, 8), a_coff=a_coff[:8], c_coff=c_coff[:8], **kw)
                flags.check_family(family_of(case, dt), what, plan)
                ref = patch2_scatter_ref(c64, *case["grid"]) if scatter else c64
                assert_bit_equal(C[:, PAD:PAD + cw], ref, what + " C")
                assert_sentinel(C, PAD, cw, what + " C")
                if C2 is not None:   # the GELU values are outside exact arithmetic; where they went is not
                    assert_sentinel(C2, PAD, cw, what + " C2")
                    assert bool(torch.isfinite(C2[:, PAD:PAD + cw].float()).all()), what + " C2: part of the slice was not written"
                if r0_64 is not None:
                    assert_bit_equal(r0, r0_64, what + " red0 (rows = samples)")
                    assert_bit_equal(r1, r1_64, what + " red1 (rows = samples)")


# ------------------------------------------------------------------------------------------------ TN cases
SPLIT_SWEEP = tuple({"tn_want": w, "tn_want2": w, "tn_fill": f} for f in (1, 0) for w in (97, 333, 768))
P2_ROUNDS = ({"tn_p2_rounds": 1}, {"tn_p2_rounds": 0})


def tn(name, M, N, K, fam, leg, hw=0, dts=BOTH, flags=({},), tr=(1, 0), **kw):
    """one weight-gradient shape W[N, K] += X[M, N]^T pro(Y)[M, K] with colsum.  kw: pro, stats (aux = W2, red0 = P), per_sample
    (b_bstride), patch = (B, gh, gw, cin): A_PATCH2 gather of Y"""
    return dict(name=name, M=M, N=N, K=K, hw=hw, fam=fam, leg=leg, dts=tuple(dts), flags=tuple(flags), tr=tuple(tr),
                pro=kw.pop("pro", R.PRO_NONE), stats=kw.pop("stats", False), per_sample=kw.pop("per_sample", False),
                patch=kw.pop("patch", None), **kw)


def _tn_patch(B, gh, gw, cin, cout, fam, leg):
    return tn(f"patch2_{B}x{gh}x{gw}_cin{cin}_cout{cout}", B * gh * gw, cout, 4 * cin, fam, leg, patch=(B, gh, gw, cin))


def tn_cases():
    """`small` = N < 96 || K < 96 || (cdiv(N, 128) cdiv(K, 128) < 24 && M < 65536) selects the 64-tiles; the lean kernel needs
    M % 32 == 0; on 128-tiles in bf16 with transposing reads (tn_tr = 1), M % 64 == 0 and M / 64 >= 2 splits it runs 64-row steps,
    on rectangular tiles where tn_rect says so"""
    g = R.PRO_GRN
    c = [
        # ---- 64-tiles
        tn("t64_generic_70x8x32", 70, 8, 32, TN_GEN, "small, M % 32 != 0: gemm_tn_kernel<64>"),
        tn("t64_generic_1000x96x40", 1000, 96, 40, TN_GEN, "small (K < 96), M % 32 != 0, several splits"),
        tn("t64_lean_512x96x40", 512, 96, 40, TN_FAST, "small, M % 32 == 0: gemm_tn_fast_kernel<64>, 32-row steps"),
        tn("t64_lean_4096x224x896", 4096, 224, 896, TN_FAST, "14 tiles of 128 and M < 65536: still `small`, 64-tiles (no rectangular tile)"),
        tn("t64_lean_4096x512x384", 4096, 512, 384, TN_FAST, "12 tiles of 128: 64-tiles"),
        tn("t64_lean_4096x896x224", 4096, 896, 224, TN_FAST, "14 tiles of 128: 64-tiles"),
        tn("t64_lean_ktail_4096x640x200", 4096, 640, 200, TN_FAST, "10 tiles of 128: 64-tiles, K % 64 = 8"),
        # ---- 128-tiles
        tn("t128_one_tile_65536x128x128", 65536, 128, 128, TN_FAST, "M >= 65536: 128-tiles; bf16 tn_tr = 1: <128, 64-row steps, 1 buffer>"),
        tn("t128_square_4096x384x1024", 4096, 384, 1024, TN_FAST, "24 tiles of 128: square 128-tiles", flags=SPLIT_SWEEP),
        tn("t128_square_ktail_4096x640x648", 4096, 640, 648, TN_FAST, "30 tiles, K % 128 = 8"),
        # ---- rectangular tiles (bf16, tn_tr = 1, tn_rect = 11; the other settings run the square 128-tiles on the same values)
        tn("rect_n_full_4096x224x1536", 4096, 224, 1536, TN_FAST, "tn_rect bit 0: N in 224 .. 256, K >= 256: <256 x 128>", flags=SPLIT_SWEEP),
        tn("rect_n_div_4096x512x768", 4096, 512, 768, TN_FAST, "tn_rect bit 1: N % 256 == 0, no prologue: <256 x 128>, two tiles along N"),
        tn("rect_n_div_4096x1536x224", 4096, 1536, 224, TN_FAST, "N % 256 == 0 wins over K in 224 .. 256 (k_full = !n_full): <256 x 128>, six tiles along N"),
        tn("rect_n_div_ktail_4096x1536x232", 4096, 1536, 232, TN_FAST, "<256 x 128>, two tiles along K, the second 104 wide"),
        tn("rect_k_full_4096x1664x224", 4096, 1664, 224, TN_FAST,
           "tn_rect bit 0: K in 224 .. 256, N >= 256, N % 256 != 0 (not n_div), 13 x 2 = 26 tiles of 128: <128 x 256>, no prologue"),
        tn("rect_k_full_ktail_4096x1664x232", 4096, 1664, 232, TN_FAST, "<128 x 256> with 24 columns of the K tile unused"),
        # ---- GRN prologue
        tn("grn_generic_300x40x160_hw100", 300, 40, 160, TN_GEN, "M % 32 != 0: generic kernel, prologue per row", hw=100, pro=g),
        tn("grn_t64_lean_1024x96x384_hw64", 1024, 96, 384, TN_FAST, "64-tiles, PRO = 1, 32-row steps", hw=64, pro=g),
        tn("grn_t128_4096x384x1024_hw256", 4096, 384, 1024, TN_FAST, "128-tiles, PRO = 1, 64-row steps (hw % 64 == 0)", hw=256, pro=g),
        tn("grn_rect_n_full_4096x224x1536_hw64", 4096, 224, 1536, TN_FAST, "<256 x 128> with PRO = 1", hw=64, pro=g),
        tn("grn_rect_k_full_4096x1536x224_hw256", 4096, 1536, 224, TN_FAST, "<128 x 256> with PRO = 1 (n_div needs no prologue, so k_full holds)",
           hw=256, pro=g),
        # ---- weight gradient with GRN statistics (bf16, tn_tr = 1 only: PRO = 2, whole samples per split)
        tn("grn_stats_1024x96x384_hw64", 1024, 96, 384, TN_FAST, "aux = W2, red0 = P: <128, PRO = 2>; one ragged N tile", hw=64, pro=g, stats=True,
           dts=(BF16,), tr=(1,), flags=P2_ROUNDS),
        tn("grn_stats_1024x136x520_hw256", 1024, 136, 520, TN_FAST, "PRO = 2 with two N tiles and a K tail", hw=256, pro=g, stats=True,
           dts=(BF16,), tr=(1,), flags=P2_ROUNDS),
        # 2 x 3 = 6 tiles, 96 samples: tn_p2_rounds = 1 gives 512 / 6 = 85 splits (11 of them own two samples), tn_p2_rounds = 0 the
        # largest divisor of 96 below 2 tn_want / 6 = 256, one sample per split; on the two shapes above both settings give one
        # sample per split (16 and 4 samples)
        tn("grn_stats_6144x256x384_hw64", 6144, 256, 384, TN_FAST, "PRO = 2, splits of one and of two whole samples", hw=64, pro=g, stats=True,
           dts=(BF16,), tr=(1,), flags=P2_ROUNDS),
        # ---- per-sample outputs (bf16, tn_tr = 1 only)
        tn("per_sample_512x96x128_hw64", 512, 96, 128, TN_FAST, "b_bstride: one split per sample, plain stores", hw=64, per_sample=True,
           dts=(BF16,), tr=(1,)),
        tn("per_sample_1024x192x136_hw256", 1024, 192, 136, TN_FAST, "b_bstride: <256 x 128> (N in 192 .. 256), ks = 4 splits per sample: atomics",
           hw=256, per_sample=True, dts=(BF16,), tr=(1,)),
        # ---- A_PATCH2 gather of Y
        _tn_patch(6, 4, 4, 32, 96, TN_FAST, "gw = 4: a 32-row step is 8 grid rows across samples"),
        _tn_patch(4, 8, 8, 16, 96, TN_FAST, "gw = 8"),
        _tn_patch(1, 4, 32, 8, 96, TN_FAST, "gw = 32: one grid row per step"),
        _tn_patch(1, 2, 64, 8, 96, TN_FAST, "gw = 64"),
        _tn_patch(1, 2, 128, 8, 96, TN_FAST, "gw = 128: a step inside one grid row"),
        _tn_patch(2, 4, 24, 8, 96, TN_GEN, "gw = 24 divides neither 32 nor by 64: generic kernel"),
        _tn_patch(2, 8, 8, 256, 384, TN_FAST, "24 tiles of 128: the gather on 128-tiles with 64-row steps"),
    ]
    return c


_TN_FIX: dict = {}


def tn_fixture(case):
    if _TN_FIX.get("name") == case["name"]:
        return _TN_FIX["fx"]
    M, N, K, hw, s0 = case["M"], case["N"], case["K"], case["hw"], _seed(case["name"])
    v = 1 if (case["stats"] and hw > 64) else 2
    fx = dict(v=v)
    fx["x"] = x = ints((M, N), -v, v, s0 + 1)
    if case["patch"]:
        B, gh, gw, cin = case["patch"]
        fx["y_src"] = ints((4 * M, cin), -v, v, s0 + 2)
        y = patch2_gather_ref(fx["y_src"], B, gh, gw)
    else:
        fx["y_src"] = y = ints((M, K), -v, v, s0 + 2)
    fx["W_old"], fx["cs_old"] = ints((N, K), -8, 8, s0 + 3), ints((N,), -8, 8, s0 + 4)
    ymax = v
    a = y
    if case["pro"] == R.PRO_GRN:
        nb = M // hw
        fx["s"], fx["beta"] = choice([0.5, 1.0, 2.0], (nb, K), s0 + 5), ints((K,), -2, 2, s0 + 6)
        a = y * fx["s"][sample_of(M, hw)] + fx["beta"][None, :]
        ymax = 2 * v + 2
    # multiples of 1/2 with the prologue: twice the integer budget
    assert_exact_precondition(2 * M, v, ymax, 8, case["name"] + " weight gradient")
    assert_exact_precondition(M, v, 1, 8, case["name"] + " colsum")
    if case["per_sample"]:
        nb = M // hw
        fx["W"] = torch.stack([x[i * hw:(i + 1) * hw].t() @ y[i * hw:(i + 1) * hw] for i in range(nb)])   # stored, not accumulated
        fx["cs"] = x.reshape(nb, hw, N).sum(1)
    else:
        fx["W"] = fx["W_old"] + x.t() @ a
        fx["cs"] = fx["cs_old"] + x.sum(0)
    if case["stats"]:
        nb = M // hw
        fx["W2"] = W2 = ints((N, K), -1, 1, s0 + 7)
        fx["P_old"] = ints((nb, K), -8, 8, s0 + 8)
        Q = torch.stack([x[i * hw:(i + 1) * hw].t() @ y[i * hw:(i + 1) * hw] for i in range(nb)])
        assert _amax(Q) <= 256, f"{case['name']}: max |Q_b| = {_amax(Q)} > 256"
        assert_exact_precondition(N, 256, 1, 8, case["name"] + " P")
        fx["P"] = fx["P_old"] + (Q * W2[None]).sum(1)   # P[b, k] = sum_hw dz g, dz = dout . W2
    _TN_FIX.clear()
    _TN_FIX.update(name=case["name"], fx=fx)
    return fx


def run_tn_case(ops, case, dt, device, flags: Flags = Flags()) -> None:
    fx = tn_fixture(case)
    M, N, K, hw = case["M"], case["N"], case["K"], case["hw"]
    f32 = lambda t: t.float().to(device).contiguous()
    ldb = N + 2 * PAD
    X = embed(fx["x"], PAD, ldb, dt, device)
    kw0 = dict(dtype=dt, pro=case["pro"], hw=hw)
    if case["patch"]:
        B, gh, gw, cin = case["patch"]
        lda = cin + 2 * PAD
        kw0.update(a_mode=R.A_PATCH2, gh=gh, gw=gw, cs=cin)
    else:
        lda = K + 2 * PAD
    Y = embed(fx["y_src"], PAD, lda, dt, device)
    if case["pro"] == R.PRO_GRN:
        kw0.update(grn_s=f32(fx["s"]), grn_b=f32(fx["beta"]))
    if case["per_sample"]:   # the packed per-sample products of the block backward: [nb, N, K]
        ldc, coff, kw0["b_bstride"] = K, 0, N * K
    else:
        ldc, coff = K + 2 * PAD, PAD
    ldx = K + PAD
    W2 = embed(fx["W2"], 0, ldx, dt, device) if case["stats"] else None
    settings = [dict(s, tn_tr=tr) for s in flags.variants(case["flags"]) for tr in (case["tr"] if dt == BF16 else case["tr"][:1])]
    if flags.lib is None:
        settings = [{}]
    for setting in settings:
        with flags.scoped(setting):
            what = f"{case['name']}[{dtname(dt)}] {setting or ''}"
            if case["per_sample"]:
                nb = M // hw
                Wb = f32(ints((nb * N, K), -8, 8, 11))       # old values: overwritten
                cs = f32(ints((nb, N), -8, 8, 12))
            else:
                Wb = torch.full((N, ldc), SENT, dtype=F32)
                Wb[:, coff:coff + K] = fx["W_old"].float()
                Wb = Wb.to(device)
                cs = f32(fx["cs_old"])
            kw = dict(kw0, colsum=cs)
            P = None
            if case["stats"]:
                assert flags.lib is None or ops.tn_grn_stats_ok(M, N, K, hw, dt), what + ": not served"
                P = f32(fx["P_old"])
                kw.update(aux=W2, ldx=ldx, red0=P)
            args = (Y, X, Wb, M, N, K, lda, ldb, ldc)
            ops.gemm("tn", *args, a_coff=[PAD], b_off=[PAD], c_coff=[coff], **kw)
            plan = None if flags.lib is None else flags.plan_of(ops, "tn", *args, a_coff=[PAD], b_off=[PAD], c_coff=[coff], **kw)
            flags.check_family(family_of(case, dt), what, plan)
            if case["per_sample"]:
                assert_bit_equal(Wb, fx["W"].reshape(-1, K), what + " per-sample products (rows = sample * N + n)")
            else:
                assert_bit_equal(Wb[:, coff:coff + K], fx["W"], what + " W")
                assert_sentinel(Wb, coff, K, what + " W")
            assert_bit_equal(cs, fx["cs"], what + " colsum")
            if P is not None:
                assert_bit_equal(P, fx["P"], what + " P (rows = samples)")


# ------------------------------------------------------------------------------------------------ data movement
def run_im2col_case(ops, dt, device, B=5, H=6, W=5, C=8) -> None:
    """im2col3x3 / col2im3x3 move data: bit equality for any values; the same 6 x 5 grid as the A_CONV3 case"""
    x = ints((B * H * W, C), -8, 8, 31)
    col = ops.im2col3x3(x.to(dt).to(device), B, H, W, C)
    assert_bit_equal(col, conv3_gather_ref(x, B, H, W), f"im2col3x3 [{dtname(dt)}]")
    d = ints((B * H * W, 9 * C), -8, 8, 32)
    # the transpose of the gather, as its action on the identity: dx[p, c] = sum over (q, t) with source(q, t) = p of d[q, t, c]
    ref = torch.zeros(B * H * W, C, dtype=torch.float64)
    src = conv3_gather_ref(torch.arange(1, B * H * W + 1, dtype=torch.float64)[:, None], B, H, W).long()   # 0 = outside
    for t in range(9):
        ok = src[:, t] > 0
        ref.index_add_(0, src[ok, t] - 1, d[ok, t * C:(t + 1) * C])
    assert_bit_equal(ops.col2im3x3(d.to(dt).to(device), B, H, W, C), ref, f"col2im3x3 [{dtname(dt)}]")


# ------------------------------------------------------------------------------------------------ depthwise 7x7
DW_SHAPES = [(1, 2, 2, 768), (2, 4, 4, 192), (1, 16, 16, 32), (1, 17, 23, 24), (2, 33, 19, 40), (1, 40, 72, 64), (5, 48, 16, 64)]
DW_SHIPPED = 15
DW_FLAGS = ({"dw_mfma": 0}, {"dw_mfma": 7}, {"dw_mfma": 15}, {"dw_mfma": 31})

_DW_FIX: dict = {}


def dw_fixture(shape):
    if _DW_FIX.get("shape") == shape:
        return _DW_FIX["fx"]
    B, H, W, C = shape
    M, s0 = B * H * W, 100 * H + W + C
    fx = dict(x=ints((M, C), -2, 2, s0 + 1), dy=ints((M, C), -2, 2, s0 + 2), add=ints((M, C), -2, 2, s0 + 3), w=ints((49, C), -2, 2, s0 + 4),
              bias=ints((C,), -8, 8, s0 + 5), dw_old=ints((49, C), -8, 8, s0 + 6), db_old=ints((C,), -8, 8, s0 + 7))
    assert_exact_precondition(49, 2, 2, 8, "depthwise forward / data gradient")
    assert_exact_precondition(2 * M, 2, 2, 8, "depthwise weight gradient, two launches")
    fx["y"] = dw_fwd_ref(fx["x"], fx["w"], fx["bias"], B, H, W, C)
    fx["y_nobias"] = fx["y"] - fx["bias"]
    fx["dx"] = dw_bwd_data_ref(fx["dy"], fx["w"], None, B, H, W, C)
    fx["dx_add"] = fx["dx"] + fx["add"]
    assert max(_amax(fx["y"]), _amax(fx["dx_add"])) <= 206   # 49 x 4 + 8 + 2 < 256: exact in bf16
    g, b = dw_bwd_weight_ref(fx["dy"], fx["x"], B, H, W, C)
    fx["dw"], fx["db"] = fx["dw_old"] + 2 * g, fx["db_old"] + 2 * b
    _DW_FIX.clear()
    _DW_FIX.update(shape=shape, fx=fx)
    return fx


def run_dw_case(ops, shape, dt, device, flags: Flags = Flags()) -> None:
    """forward (with / without bias), data gradient (with / without add), weight and bias gradient (two accumulating launches onto
    integer old values) under every value of dw_mfma: each equals the float64 statement, hence they equal each other"""
    fx = dw_fixture(shape)
    B, H, W, C = shape
    shipped = flags.get("dw_mfma")
    assert shipped is None or shipped == DW_SHIPPED, f"dw_mfma is {shipped} on entry, the shipped value is {DW_SHIPPED}"
    f32 = lambda t: t.float().to(device).contiguous()
    st = lambda t: t.to(dt).to(device)
    x, dy, add, w, bias = st(fx["x"]), st(fx["dy"]), st(fx["add"]), f32(fx["w"]), f32(fx["bias"])
    grid = (B, 1, H, W)
    for setting in (flags.variants(DW_FLAGS) if dt == BF16 else [{}]):   # the flag selects among bf16 kernels
        with flags.scoped(setting):
            what = f"dwconv7 {B}x{H}x{W}x{C}[{dtname(dt)}] {setting or ''}"
            assert_bit_equal(ops.dwconv7_fwd(x, w, bias, B, H, W, C), fx["y"], what + " forward", grid)
            assert_bit_equal(ops.dwconv7_fwd(x, w, None, B, H, W, C), fx["y_nobias"], what + " forward, no bias", grid)
            assert_bit_equal(ops.dwconv7_bwd_data(dy, w, add, B, H, W, C), fx["dx_add"], what + " data gradient + add", grid)
            assert_bit_equal(ops.dwconv7_bwd_data(dy, w, None, B, H, W, C), fx["dx"], what + " data gradient", grid)
            dw, db = f32(fx["dw_old"]), f32(fx["db_old"])
            ops.dwconv7_bwd_weight(dy, x, dw, db, B, H, W, C)
            ops.dwconv7_bwd_weight(dy, x, dw, db, B, H, W, C)
            assert_bit_equal(dw, fx["dw"], what + " weight gradient (rows = taps 7 ky + kx)")
            assert_bit_equal(db, fx["db"], what + " bias gradient")


def clear_fixtures() -> None:
    _NT_FIX.clear()
    _TN_FIX.clear()
    _DW_FIX.clear()

