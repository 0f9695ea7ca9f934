"""CPU: the exact-arithmetic fixtures of tests/ref_exact_narrow.py without a GPU.

1. the dispatch arithmetic restated in Python (blk_grid, stem_rows_per_wg, proj_wgs, the scratch sizes) says of every case what
   the table lists it for: tiles per workgroup, the clipped last workgroup, rows per workgroup, the grids past their caps;
2. the preconditions of every fixture: the budgets (every reduction's sum of magnitudes below 2^24) and the bf16 representability
   are asserted while a fixture is built, so building them all is the check; the operation counts K_BLOCK / K_PROJ are what RE derives;
3. the plain-PyTorch entry points (ref_exact_narrow.TorchEntry) pass the runners the GPU file runs on the library;
4. sensitivity: each seeded defect (ref_exact_narrow.DEFECTS, one indexing error each) fails an exact runner; what the statements and
   thresholds of tests/test_gpu_vscyto2d.py make of the same defect at that file's own shapes is recorded in OLD_TESTS_SEE and
   asserted, so the stated gap stays true."""

import pytest
import torch

from tests import ref_exact_narrow as X
from tests import ref_ops_narrow as R

CPU = "cpu"
CS = (4, 8)
DTN = tuple(X.DTYPES)


@pytest.fixture(scope="module", autouse=True)
def _release_fixtures():
    yield
    X.clear_fixtures()


def _sid(shape):
    return "x".join(map(str, shape))


# ------------------------------------------------------------------------------------------------ 1. the tables
def test_block_shapes_reach_the_launches_they_are_listed_for():
    plan = {s: X.block_plan(s) for s in X.BLOCK_SHAPES}
    assert all(plan[s]["tpw"] == 1 for s in X.BLOCK_SHAPES[:5]) and set(X.BOUNDED_SHAPES) <= set(X.BLOCK_SHAPES)
    assert plan[(1, 1, 1)]["last_pixels"] == 1 and plan[(1, 3, 5)]["nt"] == 1 and plan[(1, 16, 16)] == dict(nt=1, gps=1, tpw=1, last_tiles=1, last_pixels=256)
    assert plan[(2, 7, 37)] == dict(nt=2, gps=2, tpw=1, last_tiles=1, last_pixels=3) and 256 % 37 != 0
    assert plan[(300, 8, 257)] == dict(nt=9, gps=5, tpw=2, last_tiles=1, last_pixels=8)
    assert plan[(2049, 3, 86)] == dict(nt=2, gps=1, tpw=2, last_tiles=2, last_pixels=2)
    # the shapes of the tolerance tests: one tile per workgroup, always
    assert all(X.blk_grid(B, H * W)[1] == 1 for B, H, W in [(1, 13, 21), (3, 64, 96), (3, 128, 128), (4, 256, 256)])
    # production: a 2048^2 map walks eight tiles per workgroup, a 1024^2 map two
    assert X.blk_grid(1, 2048 * 2048) == (2048, 8) and X.blk_grid(1, 1024 * 1024)[1] == 2
    for (B, H, W), p in plan.items():
        for C in CS:
            G = B * p["gps"]
            assert [X.ws_floats(op, B, H * W, C) for op in (X.OP_FWD1, X.OP_BWD_A, X.OP_BWD_B, X.OP_BWD_C)] == \
                [G * 4 * C, G * (4 * C * C + C + 8 * C), G * (4 * C * C + 4 * C), G * 50 * C]


def test_stem_projection_and_shuffle_cases_reach_their_paths():
    cases = {c["name"]: c for c in X.stem_cases()}
    assert len(cases) == len(X.stem_cases())
    assert {(c["kernel"], c["Cin"]) for c in cases.values() if c["C0"] == 96} == {((1, 2, 2), 1), ((5, 2, 2), 1), ((1, 2, 2), 3)}
    assert X.stem_rows_per_wg(819) == 64 and 819 % 64 == 51 and X.stem_rows_per_wg(65536) == 64
    assert X.stem_rows_per_wg(257 * 256) == 128 and 257 * 256 % 128 == 0 and X.stem_rows_per_wg(257 * 257) == 128 and 257 * 257 % 128 == 1
    a, b, c = cases["limit_c128_k31"], cases["limit_c63_k64"], cases["lds_k15_c1024"]
    assert a["C0"] * (a["K"] + 1) == X.STEM_EPT * X.NB and a["C0"] == 128 and b["K"] == 64 and b["C0"] * (b["K"] + 1) <= 4096
    assert c["K"] * c["C0"] + c["C0"] == 16384 and c["K"] == 15
    big = cases["stride_1x700x1000"]
    assert big["M0"] * (big["C0"] // 4) > 65536 * X.NB == 16777216 and big["dts"] == ("fp32",)
    for name, entry, kernel, c0 in X.stem_refusals():
        K = kernel[0] * kernel[1] * kernel[2]
        for dtn, C0 in c0.items():
            if entry == "fwd":
                assert K * C0 + C0 > 16384 or C0 % X.vec_elems(X.DTYPES[dtn])
            else:
                assert sum([C0 > 128, K > 64, C0 * (K + 1) > 4096]) >= 1 and (name != "wgrad_slots" or (C0 <= 128 and K <= 64))
    assert X.ws_floats(X.OP_STEM, 1, 257 * 257, 96, 4) == 517 * 96 * 5 and X.ws_floats(X.OP_PROJ, 1, 16385, 8, 192) == 1024 * 8 * 193
    assert X.proj_wgs(16385) == 1024 and X.proj_wgs(17) == 2 and X.cdiv(X.PROJ_BIG["M"], 16) > 65536
    assert set(X.PROJ_CCAT) == {1, 15, 17, 144, 191, 192} and set(X.PROJ_M) == {1, 15, 16, 17, 16385} and 16 * X.PJ_V == 192
    assert set(X.SHUFFLE_CFG) == {(1, 1, 2, True), (1, 1, 2, False), (2, 3, 2, True), (1, 1, 3, True), (1, 5, 1, False)}
    (Cout, D, s, _), (B, h, w) = X.SHUFFLE_BIG
    assert B * h * w * Cout * D * s * s > 16777216


# ------------------------------------------------------------------------------------------------ 2. preconditions
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("shape", X.BLOCK_SHAPES, ids=_sid)
def test_block_fixtures_are_within_the_exactness_budget(shape, C):
    fx = X.block_fixture(shape, C)   # asserts the budgets and that y, out, dx hold bf16 numbers
    B = shape[0]
    assert set(fx["b1f"].abs().tolist()) == {16.0, 32.0} and bool((fx["b1f"] > 0).any()) and bool((fx["b1f"] < 0).any())
    assert torch.equal(fx["s"], fx["s"].round()) and (B == 1 or len({tuple(r.tolist()) for r in fx["s"]}) > 1)
    for k in ("x", "dw_w", "W2", "dout", "dyc", "t", "x2", "gb", "b2"):
        assert torch.equal(fx[k], fx[k].round()) and X.is_bf16(fx[k]), k
    if B * shape[1] * shape[2] > 100000:
        assert set(fx["dout"].unique().tolist()) == {-1.0, 0.0, 1.0} and float((fx["s"] == 0).double().mean()) > 0.4


@pytest.mark.parametrize("C", CS)
def test_operation_counts_are_what_the_formulas_give(C):
    ks = [X.bounded_fixture(s, C)["k"] for s in X.BOUNDED_SHAPES]
    assert all(k == X.K_BLOCK[C] for k in ks), ks
    assert all(X.bounded_fixture(s, C)["hmax"] <= 4.0 for s in X.BOUNDED_SHAPES)
    for M, Ccat in X.PROJ_BOUNDED:
        fx = X.proj_bounded_fixture(M, Ccat, C)
        assert dict(rstd=fx["rstd"].k, xn=fx["xn"].k, out=fx["out"].k) == X.K_PROJ[Ccat]
    # the rules for a library function: the argument's error through the derivative, plus its own ulp
    x = X.RE(torch.tensor([0.25, 2.0])) * X.RE(torch.tensor([3.0, 0.75]))
    r = X.fn(x, lambda v: v.rsqrt(), lambda v: 0.5 * v.pow(-1.5), X.RSQRT_ULP)
    assert r.k == x.k + 4 and bool((r.A >= r.v.abs()).all()) and X.EXP_K == 8 + 8 + 2


# ------------------------------------------------------------------------------------------------ 3. reference run
@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("shape", X.BLOCK_SHAPES, ids=_sid)
def test_block_exact_cases_on_the_reference(shape, C, dtn):
    X.run_block_exact(X.TorchEntry(), shape, C, dtn, CPU)


@pytest.mark.parametrize("dtn", DTN)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("shape", X.BOUNDED_SHAPES, ids=_sid)
def test_block_bounded_cases_on_the_reference(shape, C, dtn):
    X.run_block_bounded(X.TorchEntry(), shape, C, dtn, CPU)


@pytest.mark.parametrize("case", X.stem_cases(), ids=lambda c: c["name"])
def test_stem_cases_on_the_reference(case):
    for dtn in case["dts"]:
        X.run_stem_case(X.TorchEntry(), case, dtn, CPU)


def test_refusals_on_the_reference():
    for dtn in DTN:
        for ref in X.stem_refusals():
            X.run_stem_refusal(X.TorchEntry(), ref, dtn, CPU)
        for C in CS:
            X.run_proj_refusal(X.TorchEntry(), C, dtn, CPU)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("Ccat", X.PROJ_CCAT)
def test_projection_cases_on_the_reference(Ccat, C):
    for dtn in DTN:
        for M in X.PROJ_M:
            X.run_proj_case(X.TorchEntry(), M, Ccat, C, dtn, CPU)
        for M, cc in X.PROJ_BOUNDED:
            if cc == Ccat:
                X.run_proj_bounded(X.TorchEntry(), M, Ccat, C, dtn, CPU)


def test_grid_stride_cases_on_the_reference():
    X.run_proj_case(X.TorchEntry(), X.PROJ_BIG["M"], X.PROJ_BIG["Ccat"], X.PROJ_BIG["C"], "fp32", CPU, bwd=False)
    X.run_shuffle_case(X.TorchEntry(), *X.SHUFFLE_BIG, "fp32", CPU)


def test_shuffle_cases_on_the_reference():
    for cfg in X.SHUFFLE_CFG:
        for geo in X.SHUFFLE_GEO:
            for dtn in DTN:
                X.run_shuffle_case(X.TorchEntry(), cfg, geo, dtn, CPU)


# ------------------------------------------------------------------------------------------------ 4. seeded defects
class _Ops:
    """the call surface of viscy_amd.ops.narrow_* on an object with the ten entry points (CPU tensors)"""

    def __init__(self, ep):
        self.ep = ep

    @staticmethod
    def _new(shape, dt):
        return torch.full(tuple(shape), float("nan"), dtype=dt)

    def narrow_block_fwd1(self, x, dw_w, dw_b, W1f, b1f, colsq, B, H, W, C):
        y = self._new(x.shape, x.dtype)
        assert self.ep.block_fwd1(x, dw_w, dw_b, W1f, b1f, y, colsq, B, H, W) == 0
        return y

    def narrow_block_fwd2(self, y, x, W1f, b1f, s, gb, W2, b2, B, H, W, C):
        out = self._new(x.shape, x.dtype)
        assert self.ep.block_fwd2(y, x, W1f, b1f, s, gb, W2, b2, out, B, H, W) == 0
        return out

    def narrow_block_bwd_a(self, dout, y, W1f, b1f, s, gb, W2, dW2, db2, P, S, B, H, W, C):
        assert self.ep.block_bwd_a(dout, y, W1f, b1f, s, gb, W2, dW2, db2, P, S, B, H, W) == 0

    def narrow_block_bwd_b(self, dout, y, W1f, b1f, s, t, W2, dW1f, db1f, B, H, W, C):
        dy = self._new(y.shape, y.dtype)
        assert self.ep.block_bwd_b(dout, y, W1f, b1f, s, t, W2, dy, dW1f, db1f, B, H, W) == 0
        return dy

    def narrow_block_bwd_c(self, dy, x, dout, dw_w, ddw, ddb, B, H, W, C):
        dx = self._new(x.shape, x.dtype)
        assert self.ep.block_bwd_c(dy, x, dout, dw_w, dx, ddw, ddb, B, H, W) == 0
        return dx

    def narrow_proj_fwd(self, cat, gamma, beta, Wp, bp, M, Ccat, C):
        out, mean, rstd = self._new((M, C), cat.dtype), self._new((M,), torch.float32), self._new((M,), torch.float32)
        assert self.ep.proj_fwd(cat, gamma, beta, Wp, bp, out, mean, rstd) == 0
        return out, mean, rstd

    def narrow_proj_bwd(self, d, cat, mean, rstd, gamma, beta, Wp, dW, db, M, Ccat, C):
        dxn = self._new((M, Ccat), cat.dtype)
        assert self.ep.proj_bwd(d, cat, mean, rstd, gamma, beta, Wp, dxn, dW, db) == 0
        return dxn

    def narrow_stem_fwd(self, x, W, b, kernel, dt):
        B, _, _, H, Wd = x.shape
        out = self._new((B * (H // kernel[1]) * (Wd // kernel[2]), W.shape[0]), dt)
        assert self.ep.stem_fwd(x, W, b, out, kernel) == 0
        return out

    def narrow_stem_wgrad(self, x, df, dW, db, kernel):
        assert self.ep.stem_wgrad(x, df, dW.view(dW.shape[0], -1), db, kernel) == 0

    def narrow_voxel_shuffle_bwd(self, dout, B, h, w, Cout, D, s, pool, dt):
        df = self._new((B * h * w, Cout * D * s * s), dt)
        assert self.ep.shuffle_bwd(dout, df, B, h, w, Cout, D, s, pool) == 0
        return df


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


OLD_SHAPES = [(1, 13, 21), (3, 64, 96), (3, 128, 128)]
OLD_COMBOS = [(4, "fp32"), (8, "bf16")]


def _old_block_criteria(ops, shape, C, dtn) -> list:
    """test_narrow_block_ops_match_torch of tests/test_gpu_vscyto2d.py, statement by statement; the assertions that fail"""
    dt = X.DTYPES[dtn]
    tol = 2e-4 if dt == torch.float32 else 2.5e-2
    B, H, W = shape
    M, HD = B * H * W, 4 * C
    g = torch.Generator().manual_seed(C * 100 + H)
    rnd = lambda *s, sc=1.0: (torch.randn(s, generator=g) * sc)  # noqa: E731
    x = rnd(M, C).to(dt)
    dw_w, dw_b = rnd(49, C, sc=0.2), rnd(C, sc=0.1)
    W1f, b1f = rnd(HD, C, sc=0.4).to(dt), rnd(HD, sc=0.1)
    W2, b2 = rnd(C, HD, sc=0.3).to(dt), rnd(C, sc=0.1)
    grn_w, grn_b = rnd(HD, sc=0.5), rnd(HD, sc=0.1)
    dout = rnd(M, C).to(dt)
    fails = []
    chk = lambda name, ok: None if ok else fails.append(name)  # noqa: E731
    cs_r, cs = torch.zeros(B, HD), torch.zeros(B, HD)
    y_r = R.narrow_block_fwd1(x, dw_w, dw_b, W1f, b1f, cs_r, B, H, W, C)
    y = ops.narrow_block_fwd1(x, dw_w, dw_b, W1f, b1f, cs, B, H, W, C)
    chk("y", _rel(y, y_r) < tol)
    chk("cs", _rel(cs, cs_r) < (1e-4 if dt == torch.float32 else 2e-2))
    s = R.grn_scale(cs, grn_w)
    out_r = R.narrow_block_fwd2(y, x, W1f, b1f, s, grn_b, W2, b2, B, H, W, C)
    chk("out", _rel(ops.narrow_block_fwd2(y, x, W1f, b1f, s, grn_b, W2, b2, B, H, W, C), out_r) < tol)
    ref = [torch.zeros(C, HD), torch.zeros(C), torch.zeros(B, HD), torch.zeros(B, HD)]
    R.narrow_block_bwd_a(dout, y, W1f, b1f, s, grn_b, W2, *ref, B, H, W, C)
    got = [torch.zeros_like(t) for t in ref]
    ops.narrow_block_bwd_a(dout, y, W1f, b1f, s, grn_b, W2, *got, B, H, W, C)
    for n, a, b in zip(("dW2", "db2", "P", "S"), got, ref):
        chk(n, _rel(a, b) < 1e-4)
    t = torch.randn(B, HD, generator=g) * 0.01
    rb, gb = [torch.zeros(HD, C), torch.zeros(HD)], [torch.zeros(HD, C), torch.zeros(HD)]
    dy_r = R.narrow_block_bwd_b(dout, y, W1f, b1f, s, t, W2, *rb, B, H, W, C)
    dy = ops.narrow_block_bwd_b(dout, y, W1f, b1f, s, t, W2, *gb, B, H, W, C)
    chk("dy", _rel(dy, dy_r) < tol)
    for n, a, b in zip(("dW1f", "db1f"), gb, rb):
        chk(n, _rel(a, b) < 1e-4)
    rc, gc = [torch.zeros(49, C), torch.zeros(C)], [torch.zeros(49, C), torch.zeros(C)]
    dx_r = R.narrow_block_bwd_c(dy, x, dout, dw_w, *rc, B, H, W, C)
    dx = ops.narrow_block_bwd_c(dy, x, dout, dw_w, *gc, B, H, W, C)
    chk("dx", _rel(dx, dx_r) < tol)
    for n, a, b in zip(("ddw", "ddb"), gc, rc):
        chk(n, _rel(a, b) < 1e-4)
    return fails


def _old_proj_stem_head_criteria(ops, shape, C, dtn) -> list:
    """test_narrow_proj_stem_head_ops_match_torch of tests/test_gpu_vscyto2d.py; the assertions that fail"""
    dt = X.DTYPES[dtn]
    tol = 2e-4 if dt == torch.float32 else 2.5e-2
    B, H, W = shape
    M, Ccat = B * H * W, 144
    g = torch.Generator().manual_seed(7 + C)
    cat = (torch.randn(M, Ccat, generator=g) * 2 + 0.5).to(dt)
    gam, bet = torch.randn(Ccat, generator=g) * 0.3 + 1, torch.randn(Ccat, generator=g) * 0.1
    Wp, bp = torch.randn(C, Ccat, 1, 1, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    fails = []
    chk = lambda name, ok: None if ok else fails.append(name)  # noqa: E731
    out_r, mean_r, rstd_r = R.narrow_proj_fwd(cat, gam, bet, Wp, bp, M, Ccat, C)
    out, mean, rstd = ops.narrow_proj_fwd(cat, gam, bet, Wp, bp, M, Ccat, C)
    chk("proj_out", _rel(out, out_r) < tol and _rel(mean, mean_r) < 1e-5 and _rel(rstd, rstd_r) < 1e-4)
    d = torch.randn(M, C, generator=g).to(dt)
    dW_r, db_r = torch.zeros(C, Ccat, 1, 1), torch.zeros(C)
    dxn_r = R.narrow_proj_bwd(d, cat, mean, rstd, gam, bet, Wp, dW_r, db_r, M, Ccat, C)
    dW, db = torch.zeros(C, Ccat, 1, 1), torch.zeros(C)
    dxn = ops.narrow_proj_bwd(d, cat, mean, rstd, gam, bet, Wp, dW, db, M, Ccat, C)
    chk("proj_bwd", _rel(dxn, dxn_r) < tol and _rel(dW, dW_r) < 1e-4 and _rel(db, db_r) < 1e-4)
    xs = torch.randn(B, 1, 1, 2 * H, 2 * W, generator=g)
    Ws, bs = torch.randn(96, 1, 2, 2, generator=g), torch.randn(96, generator=g)
    chk("stem_fwd", _rel(ops.narrow_stem_fwd(xs, Ws, bs, (1, 2, 2), dt), R.narrow_stem_fwd(xs, Ws, bs, (1, 2, 2), dt)) < tol)
    df = torch.randn(M, 96, generator=g).to(dt)
    gw_r, gb_r, gw, gbias = torch.zeros(96, 1, 2, 2), torch.zeros(96), torch.zeros(96, 1, 2, 2), torch.zeros(96)
    R.narrow_stem_wgrad(xs, df, gw_r, gb_r, (1, 2, 2))
    ops.narrow_stem_wgrad(xs, df, gw, gbias, (1, 2, 2))
    chk("stem_wgrad", _rel(gw, gw_r) < 1e-4 and _rel(gbias, gb_r) < 1e-4)
    dout = torch.randn(B, 1, 1, 2 * H, 2 * W, generator=g)
    chk("shuffle", _rel(ops.narrow_voxel_shuffle_bwd(dout, B, H, W, 1, 1, 2, True, dt), R.narrow_voxel_shuffle_bwd(dout, B, H, W, 1, 1, 2, True, dt)) < tol)
    return fails


def _old_criteria(ep, which: str) -> dict:
    """{shape: failing assertions} of the tolerance tests at their own shapes, over OLD_COMBOS; shapes that pass are left out"""
    run, see = (_old_block_criteria if which == "block" else _old_proj_stem_head_criteria), {}
    for shape in OLD_SHAPES:
        f = sorted({n for C, dtn in OLD_COMBOS for n in run(_Ops(ep), shape, C, dtn)})
        if f:
            see[shape] = f
    return see


def test_the_reference_passes_the_tolerance_tests_statements():
    assert _old_criteria(X.TorchEntry(), "block") == {} and _old_criteria(X.TorchEntry(), "other") == {}


def _exact_runner_fails(defect: str) -> str:
    """the first exact runner that fails on the defect, with the case it fails at"""
    ep = X.TorchEntry(defect)
    runs = {
        "block": [(f"run_block_exact {s}", lambda s=s: X.run_block_exact(ep, s, 4, "fp32", CPU)) for s in X.BLOCK_SHAPES],
        "proj": [(f"run_proj_case Ccat = {c}", lambda c=c: X.run_proj_case(ep, 17, c, 4, "bf16", CPU)) for c in X.PROJ_CCAT],
        "stem": [(f"run_stem_case {c['name']}", lambda c=c: X.run_stem_case(ep, c, "fp32", CPU)) for c in X.stem_cases()[:4]],
        "shuffle": [(f"run_shuffle_case {cfg} {geo}", lambda cfg=cfg, geo=geo: X.run_shuffle_case(ep, cfg, geo, "fp32", CPU))
                    for cfg in X.SHUFFLE_CFG for geo in X.SHUFFLE_GEO[:2]],
    }[OLD_TESTS_SEE[defect][0]]
    for label, run in runs:
        try:
            run()
        except AssertionError as e:
            return f"{label}: {str(e)[:200]}"
    return ""


# defect -> (family, the first exact case that fails and what it says, {shape: assertions} of the tolerance tests that fail)
OLD_TESTS_SEE = {
    "ddw_last_tile_left_out": ("block", "block_bwd_c ddw", {(1, 13, 21): ["ddw"]}),            # 64 x 96 and 128 x 128 are whole tiles
    "second_tile_skipped": ("block", "(300, 8, 257): block_fwd1 y", {}),                        # tpw == 1 at every shape of that file
    "s_of_sample_0": ("block", "(2, 7, 37): block_fwd2 out", {(3, 64, 96): ["dW1f", "dW2", "db1f", "dy", "out"],
                                                             (3, 128, 128): ["dW1f", "dW2", "db1f", "dy", "out"]}),
    "bwd_c_taps_transposed": ("block", "(1, 3, 5): block_bwd_c dx", {s: ["dx"] for s in OLD_SHAPES}),   # ddw, the other output, passes
    "proj_k176_dropped": ("proj", "Ccat = 191: proj_fwd out", {}),                              # Ccat = 144 there
    "stem_row_tail_dropped": ("stem", "stem_wgrad", {(1, 13, 21): ["stem_wgrad"]}),             # 18432 and 49152 rows are whole steps
    "pool_right_edge_unclipped": ("shuffle", "voxel_shuffle_bwd", {s: ["shuffle"] for s in OLD_SHAPES}),
}


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_seeded_defect_fails_the_exact_runner_and_what_the_tolerance_tests_see(defect):
    family, says, old = OLD_TESTS_SEE[defect]
    msg = _exact_runner_fails(defect)
    assert msg and says in msg, msg
    assert _old_criteria(X.TorchEntry(defect), "block" if family == "block" else "other") == old


def test_defect_table_is_complete():
    assert set(OLD_TESTS_SEE) == set(X.DEFECTS)
    assert sorted(d for d, v in OLD_TESTS_SEE.items() if not v[2]) == ["proj_k176_dropped", "second_tile_skipped"]
