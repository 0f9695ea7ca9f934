"""CPU: the exact-arithmetic GEMM / depthwise fixtures of tests/ref_exact_gemm.py without a GPU.

1. every case of the tables runs through the plain-PyTorch statements of tests/ref_ops.py in fp32 and bf16 and is bit-equal to
   the float64 statement: this checks the statements against a second formulation, the exactness budgets and the max |c| <= 256
   conditions;
2. the tables reach what they claim to reach: dtypes, flag settings, every generic tile width, the BK = 128 leg, the lean
   kernel's K tails / patch gather and scatter / two samples per tile / BK = 64 instantiations, the three gemm_nt2 tile widths,
   the 64-, 128- and both rectangular TN tiles (asked of vsx_gemm_plan), split sweeps, statistics and per-sample forms;
3. sensitivity: the reference namespace wrapped in mutants, each of which makes ONE subtle indexing error, fails the runner;
4. the same mutants pass ``close()`` of tests/test_gpu_ops.py on that file's random operands: the gap these tests close."""

import types

import pytest
import torch

from tests import ref_exact_gemm as X
from tests import ref_ops as R

CPU = torch.device("cpu")


def _by_dtype(cases):
    return [pytest.param(c, dt, id=f"{c['name']}-{X.dtname(dt)}") for c in cases for dt in X.BOTH]


# ------------------------------------------------------------------------------------------------ 1. reference run
@pytest.mark.parametrize("case,dt", _by_dtype(X.nt_cases()))
def test_nt_cases_on_the_reference(case, dt):
    X.run_nt_case(R, case, dt, CPU)


@pytest.mark.parametrize("case,dt", _by_dtype(X.tn_cases()))
def test_tn_cases_on_the_reference(case, dt):
    X.run_tn_case(R, case, dt, CPU)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_patch_matrices_on_the_reference(dt):
    X.run_im2col_case(R, dt, CPU)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
@pytest.mark.parametrize("shape", X.DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv7_cases_on_the_reference(shape, dt):
    X.run_dw_case(R, shape, dt, CPU)


# ------------------------------------------------------------------------------------------------ 2. the tables
def test_case_tables_are_well_formed():
    nt, tn = X.nt_cases(), X.tn_cases()
    for cases in (nt, tn):
        names = [c["name"] for c in cases]
        assert len(set(names)) == len(names)
        for c in cases:
            fams = [c["fam"]] if isinstance(c["fam"], str) else list(c["fam"].values())
            assert all(f in (X.NT2, X.NT_FAST, X.NT_GEN, X.TN_FAST, X.TN_GEN) for f in fams), c["name"]
            assert c["leg"] and c["dts"] and c["flags"], c["name"]
            vn = 8 if X.BF16 in c["dts"] else 4
            assert c["N"] % vn == 0 and c["K"] % vn == 0, c["name"]
    fam = lambda cases, f: [c for c in cases if c["fam"] == f]
    # NT: the legs of the issue
    gen = fam(nt, X.NT_GEN)
    assert {8, 16, 24, 32, 40, 64, 72} <= {c["N"] for c in gen} and {8, 130, 200} <= {c["M"] for c in gen}
    assert {8, 40, 72} <= {c["K"] for c in gen} and {4, 100} <= {c["hw"] for c in gen}
    assert [c for c in gen if c["K"] >= 256 and c["N"] > 64 and c["dts"] == (X.BF16,)], "generic BK = 128 leg"
    lean = fam(nt, X.NT_FAST)
    assert [c for c in lean if c["K"] < 256 and c["K"] % 32 == 0] and {72, 200} <= {c["K"] for c in lean}
    assert [c for c in lean if c["a_mode"] == R.A_PATCH2 and c["cs"] % 32 == 0] and [c for c in lean if c["c_mode"] == R.A_PATCH2]
    assert [c for c in lean if c["hw"] == 64 and (c["M"] // 64) % 2 == 1 and "dz" in c["epis"]]
    wide = [c for c in lean if {"nt_wide": 1} in c["flags"] and {"nt_wide": 2} in c["flags"]]
    assert wide and all(-(-c["M"] // 128) * -(-c["N"] // 128) >= 512 and c["K"] % 64 == 0 and c["K"] >= 256 for c in wide)
    g2 = fam(nt, X.NT2)
    assert all(c["M"] % 256 == 0 and c["dts"] == (X.BF16,) and c["K"] in (64, 96) for c in g2)
    assert {128, 384, 448, 896} <= {c["N"] for c in g2} and {64, 128, 256} <= {c["hw"] for c in g2}
    assert [c for c in g2 if c["pro"] == R.PRO_GRN] and [c for c in g2 if c["bstride"] and c["hw"] == 256]
    assert any("dz" in c["epis"] for c in g2) and any("res_rscale" in c["epis"] for c in g2)
    assert [c for c in nt if c["a_mode"] == R.A_CONV3 and c["nz"] == 5 and c["grid"][1:] == (6, 5)]
    used = {e for c in nt for e in c["epis"]}
    assert used == set(X.EPIS)
    # TN
    shapes = {(c["M"], c["N"], c["K"]) for c in tn}
    assert {(70, 8, 32), (1000, 96, 40), (65536, 128, 128), (4096, 384, 1024), (4096, 224, 896), (4096, 512, 384), (4096, 896, 224),
            (4096, 640, 200)} <= shapes
    assert len([c for c in tn if c["flags"] == X.SPLIT_SWEEP]) == 2
    assert {(w["tn_want"], w["tn_fill"]) for w in X.SPLIT_SWEEP} == {(w, f) for w in (97, 333, 768) for f in (0, 1)}
    assert {c["hw"] for c in tn if c["pro"] == R.PRO_GRN and not c["stats"]} >= {64, 100, 256}
    assert all(c["flags"] == X.P2_ROUNDS and c["dts"] == (X.BF16,) for c in tn if c["stats"])
    assert all(c["hw"] % 64 == 0 and c["N"] >= 96 and c["K"] >= 96 for c in tn if c["per_sample"])
    assert {c["patch"][2] for c in tn if c["patch"]} >= {4, 8, 24, 32, 64, 128}
    assert all((c["M"] % 32 != 0 or bool(c["patch"] and c["patch"][2] == 24)) == (c["fam"] == X.TN_GEN) for c in tn)
    assert max(c["M"] * max(c["N"], c["K"]) for c in tn) == 65536 * 128
    # which tile a bf16 launch with transposing reads gets, as shipped: asked of the library's own planner (vsx_gemm_plan)
    import ctypes

    from tests import gemm_plan_rows as G
    from viscy_amd import _lib

    def tile(c):
        arr, plan = G.struct_array([G.tn_case_row(c)]), _lib.VsxGemmPlan()
        assert _lib.lib().vsx_gemm_plan(G.TN, arr, G.BF16, ctypes.byref(plan)) == 0, c["name"]
        return str(plan.tile[0]) if plan.tile[0] == plan.tile[1] else f"{plan.tile[0]}x{plan.tile[1]}"
    plain = [c for c in tn if not (c["stats"] or c["per_sample"] or c["patch"])]
    for c in plain:
        want = {"t64": "64", "t128": "128", "rect_n": "256x128", "rect_k": "128x256"}
        key = next(k for k in want if k in c["name"]) if c["pro"] == R.PRO_NONE or "rect" in c["name"] or "t128" in c["name"] else "t64"
        assert tile(c) == want[key], (c["name"], tile(c))
    for t in ("256x128", "128x256"):   # each rectangular tile without and with the GRN prologue; a K tail on each
        assert {c["pro"] for c in plain if tile(c) == t} == {R.PRO_NONE, R.PRO_GRN}, t
    assert [c for c in plain if tile(c) == "128x256" and c["K"] % 256 and c["K"] != 224 and c["pro"] == R.PRO_NONE]
    assert [c for c in plain if tile(c) == "256x128" and c["K"] % 128]
    assert [c for c in plain if tile(c) == "256x128" and 224 <= c["N"] <= 256] and [c for c in plain if tile(c) == "256x128" and c["N"] % 256 == 0]
    # the statistics sweep changes the grid on at least one shape: more samples than tn_p2_rounds = 1 gives splits
    assert [c for c in tn if c["stats"] and c["M"] // c["hw"] > 512 // (-(-c["N"] // 128) * -(-c["K"] // 128))]


def test_operands_are_embedded_between_sentinels():
    """what the runners hand to the op: slices of wider buffers, NaN where the kernel must write, old integers where it adds"""
    seen = {}

    def gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw):
        seen.update(kind=kind, lda=lda, ldb=ldb, ldc=ldc, a_coff=kw["a_coff"], c_coff=kw["c_coff"], C=C.clone(), A=A.clone())
        return R.gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw)

    ns = _mutant(gemm=gemm)
    case = next(c for c in X.nt_cases() if c["name"] == "generic_200x24x40_hw100")
    X.run_nt_case(ns, dict(case, epis=("res",)), X.F32, CPU)
    assert seen["lda"] > 40 and seen["ldb"] > 40 and seen["ldc"] > 24 and seen["a_coff"][0] > 0 and seen["c_coff"][0] > 0
    assert all(v % 8 == 0 for v in (seen["lda"], seen["ldb"], seen["ldc"]))
    c0 = seen["c_coff"][0]
    assert bool(torch.isnan(seen["C"][:, c0:c0 + 24]).all()) and bool((seen["C"][:, :c0] == X.SENT).all())
    assert bool((seen["A"][:, :seen["a_coff"][0]] == X.SENT).all())
    X.run_tn_case(ns, next(c for c in X.tn_cases() if c["name"] == "t64_generic_70x8x32"), X.F32, CPU)
    c0 = seen["c_coff"][0]
    W = seen["C"]
    assert seen["kind"] == "tn" and c0 > 0 and bool((W[:, :c0] == X.SENT).all()) and float(W[:, c0:c0 + 32].abs().max()) <= 8
    assert torch.equal(W[:, c0:c0 + 32], W[:, c0:c0 + 32].round()) and float(W[:, c0:c0 + 32].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2b. the dispatch
def _instantiations():
    """every kernel instantiation the GEMM dispatch can launch, as (family, esize, tile0, tile1, step, nbuf, pro_kind, tr, epi)"""
    s = set()
    for es, trs in ((2, (1, 0)), (4, (0,))):
        for tr in trs:
            for bt in (64, 128):
                s.add((X.TN_GEN, es, bt, bt, 0, 0, 0, tr, 0))
                s.update((X.TN_FAST, es, bt, bt, 32, 2, pro, tr, 0) for pro in (0, 1))
            if es == 2:
                s.update((X.TN_FAST, 2, 128, 128, 64, 1, pro, tr, 0) for pro in (0, 1))
    s.update((X.TN_FAST, 2, tn, tk, 64, 1, pro, 1, 0) for tn, tk in ((256, 128), (128, 256)) for pro in (0, 1))
    s.add((X.TN_FAST, 2, 128, 128, 64, 1, 2, 1, 0))
    for es in (2, 4):
        s.update((X.NT_GEN, es, 128, bn, 32, 2, 0, 0, 0) for bn in (128, 64, 32, 16))
        for bk, nbuf in (((64, 1), (64, 2), (32, 1), (32, 2)) if es == 2 else ((32, 2),)):
            s.update((X.NT_FAST, es, 128, 128, bk, nbuf, pro, 0, epi) for pro in (0, 1) for epi in range(5))
    s.add((X.NT_GEN, 2, 128, 128, 128, 2, 0, 0, 0))
    for bn in (128, 256, 384):
        s.update((X.NT2, 2, 256, bn, 32, 3, 0, 0, epi) for epi in range(5))
        s.update((X.NT2, 2, 256, bn, 32, 3, 1, 0, epi) for epi in (R.EPI_NONE, R.EPI_BIAS_RES))
    s.update((X.NT2, 2, 256, bn, 32, 3, 0, 0, 6) for bn in (128, 256))   # VSX_EPI_LN_BWD
    return s


def test_plans_equal_the_recorded_dispatch():
    """vsx_gemm_plan on every row of tests/gemm_plan_rows.py against tests/golden/gemm_plan_table.json, which holds what the launch
    sites of the commit before the plan / run split did for the same rows (family, template arguments, grid, the bits in ``pro``,
    zero-fills, fixed-order sums; return code and error text of a refusal): no row differs, none is left out, and the table
    reaches every one of that commit's instantiations (27 TN, 59 NT, 23 gemm_nt2)."""
    import base64
    import json
    import lzma
    import os

    import numpy as np

    from tests import gemm_plan_rows as G
    from viscy_amd import _lib

    table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "gemm_plan_table.json")))
    assert tuple(table["fields"]) == G.FIELDS
    lib = _lib.lib()
    if not os.environ.get("VSX_FLAGS"):
        assert all(lib.vsx_get_flag(f.encode()) == v for f, v in G.SHIPPED.items())
    got, strings = G.walk_plans(lib)
    unpack = lambda pieces, dt: np.frombuffer(lzma.decompress(base64.b64decode("".join(pieces))), dtype=dt)
    idx = unpack(table["rows"], "<u2")
    codes = unpack(table["codes"], "<i8").reshape(len(G.FIELDS), table["n_codes"]).T
    assert len(idx) == table["n_rows"] == len(got) > 1_000_000
    want = codes[idx]
    text = {s: i for i, s in enumerate(table["strings"])}
    got[:, 1] = np.array([text.get(s, -1) for s in strings])[got[:, 1]]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), [(int(i), dict(zip(G.FIELDS, got[i].tolist())), dict(zip(G.FIELDS, want[i].tolist()))) for i in bad[:5]])
    codes = codes.tolist()
    launched = {(table["strings"][c[1]], *c[2:10]) for c in codes if c[0] == 0}
    assert launched == _instantiations() and len(launched) == 27 + 59 + 23
    refusals = {table["strings"][c[1]] for c in codes if c[0] != 0}
    assert len(refusals) >= 25 and all(c[0] == 1 for c in codes if c[0] != 0)


def test_plans_under_a_det_scope_equal_the_plans_under_the_flag():
    """the `det_reduce` rows of the table: with the flag at 0 and the calling thread's vsx_det_scope open, every plan is the one
    the flag gives (family, tiles, grid, fixed-order floats; return code of a refusal)"""
    import ctypes as C

    from tests import gemm_plan_rows as G
    from viscy_amd import _lib

    lib = _lib.lib()
    flag0 = lib.vsx_get_flag(b"det_reduce")
    n_det = 0
    try:
        for kind, setting, dt, rows in G._grid_groups():
            if setting != {"det_reduce": 1}:
                continue
            arr = G.struct_array(rows)
            got = []
            for flag, scope in ((1, 0), (0, 1)):
                lib.vsx_set_flag(b"det_reduce", flag)
                assert lib.vsx_det_scope(scope) == 0
                plans, rcs = (_lib.VsxGemmPlan * len(rows))(), []
                for p, pl in zip(arr, plans):
                    rcs.append(lib.vsx_gemm_plan(kind, C.byref(p), dt, C.byref(pl)))
                lib.vsx_det_scope(0)
                got.append((rcs, bytes(plans)))
                n_det += sum(pl.det_floats > 0 for pl in plans)
            assert got[0] == got[1], (kind, dt)
    finally:
        lib.vsx_det_scope(0)
        lib.vsx_set_flag(b"det_reduce", flag0)
    assert n_det > 100


# ------------------------------------------------------------------------------------------------ 3. sensitivity
def _mutant(**over):
    ns = types.SimpleNamespace(**{k: getattr(R, k) for k in dir(R) if not k.startswith("__")})
    ns.__dict__.update(over)
    return ns


def drops_last_k_of_last_row():
    """the product a[M - 1, K - 1] w[:, K - 1] is missing: a K tail or the last chunk of a zero-filled slab"""
    def gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw):
        if kind == "nt":
            A = A.clone()
            A.reshape(-1, lda)[M - 1, (kw.get("a_coff") or [0])[0] + K - 1] = 0
        return R.gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw)
    return _mutant(gemm=gemm)


def skips_last_row_of_tn():
    """the last pixel row is owned by no split"""
    def gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw):
        return R.gemm(kind, A, B, C, M - 1 if kind == "tn" else M, N, K, lda, ldb, ldc, **kw)
    return _mutant(gemm=gemm)


def credits_last_row_of_red1_to_next_sample():
    """the last row of sample 0 is added to red1 of sample 1"""
    def gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw):
        R.gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw)
        if kind == "nt" and kw.get("epi") == R.EPI_DZ and M > kw["hw"]:
            c0 = (kw.get("c_coff") or [0])[0]
            row = C.reshape(-1, ldc)[kw["hw"] - 1, c0:c0 + N].float()
            kw["red1"][0] -= row
            kw["red1"][1] += row
    return _mutant(gemm=gemm)


def shifts_one_tap_at_the_right_border():
    """at the last image column the tap (ky 3, kx 2) reads x - 2 instead of x - 1"""
    def dwconv7_fwd(x, w, bias, B, H, W, C):
        y = R.dwconv7_fwd(x, w, bias, B, H, W, C).float().view(B, H, W, C)
        xv = x.float().view(B, H, W, C)
        y[:, :, W - 1, :] += w[3 * 7 + 2] * (xv[:, :, W - 3, :] - xv[:, :, W - 2, :])
        return y.view(B * H * W, C).to(x.dtype)
    return _mutant(dwconv7_fwd=dwconv7_fwd)


def writes_one_element_outside_the_slice():
    def gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw):
        R.gemm(kind, A, B, C, M, N, K, lda, ldb, ldc, **kw)
        if kind == "nt":
            C.reshape(-1, ldc)[M - 1, (kw.get("c_coff") or [0])[0] + N] = 0
    return _mutant(gemm=gemm)


def _nt_case(name, epis):
    return dict(next(c for c in X.nt_cases() if c["name"] == name), epis=epis)


def _tn_case(name):
    return next(c for c in X.tn_cases() if c["name"] == name)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_exact_runner_catches_a_dropped_product(dt):
    for name in ("lean_ktail_200x96x72_hw128", "lean_bk32_384x192x224_hw128", "gen2_bn256_512x448x64_hw256"):
        case = _nt_case(name, ("none",))
        fx = X.nt_fixture(case)
        assert fx["a_src"][-1, -1] != 0 and X._amax(fx["w"][:, -1]) > 0, "the mutant would change nothing"
        X.run_nt_case(R, case, dt, CPU)
        with pytest.raises(AssertionError, match="elements differ"):
            X.run_nt_case(drops_last_k_of_last_row(), case, dt, CPU)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_exact_runner_catches_a_skipped_row_of_a_weight_gradient(dt):
    for name in ("t64_lean_512x96x40", "t128_one_tile_65536x128x128", "rect_n_full_4096x224x1536"):
        with pytest.raises(AssertionError, match="elements differ"):
            X.run_tn_case(skips_last_row_of_tn(), _tn_case(name), dt, CPU)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_exact_runner_catches_statistics_on_the_neighbouring_sample(dt):
    for name in ("lean_two_samples_per_tile_448x192x224_hw64", "generic_200x24x40_hw100", "gen2_bn384_512x384x96_hw64"):
        case = _nt_case(name, ("dz",))
        X.run_nt_case(R, case, dt, CPU)
        with pytest.raises(AssertionError, match="red1"):
            X.run_nt_case(credits_last_row_of_red1_to_next_sample(), case, dt, CPU)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_exact_runner_catches_a_shifted_depthwise_tap(dt):
    for shape in ((1, 17, 23, 24), (1, 16, 16, 32)):
        with pytest.raises(AssertionError, match="forward"):
            X.run_dw_case(shifts_one_tap_at_the_right_border(), shape, dt, CPU)


@pytest.mark.parametrize("dt", X.BOTH, ids=X.dtname)
def test_exact_runner_catches_a_write_outside_the_slice(dt):
    case = _nt_case("generic_200x24x40_hw100", ("bias",))
    with pytest.raises(AssertionError, match="outside the slice"):
        X.run_nt_case(writes_one_element_outside_the_slice(), case, dt, CPU)


def test_family_check_reports_a_moved_dispatch():
    """a case whose launch went to another kernel family fails and says so"""
    class Lib:
        def vsx_last_kernel(self):
            return b"gemm_nt_generic"

    with pytest.raises(AssertionError, match="dispatch has moved"):
        X.Flags(Lib()).check_family(X.NT_FAST, "case")
    X.Flags(Lib()).check_family(X.NT_GEN, "case")


# ------------------------------------------------------------------------------------------------ 4. the gap
def test_tolerance_tests_miss_the_mutants():
    """The first three mutants on the random-normal operands of tests/test_gpu_ops.py pass its ``close()`` bar (bf16: a max-norm
    error of 2e-2 of the tensor's largest value).  A dropped product moves an output by about 1 / sqrt(K) of a typical value, a
    dropped row by 1 / sqrt(M), a row of statistics by 1 / sqrt(hw); each is a bit mismatch in the exact runner.
    a. K = 1536, the (1024, 384, 1536, 1024) row of NT2_CASES: 1.3e-2.  (At K = 512 of GEMM_CASES the same mutant happens to
       exceed the bar, 3.1e-2: the tolerance test sees it or not by the luck of one operand value.)
    b. M = 32768, an M of test_gemm_tn_any_split_count: 8e-3.
    c. the per-sample statistics.  At every NT shape of GEMM_CASES / NT2_CASES the samples are short (hw <= 1024) and ``close()``
       does see this mutant (4e-2 .. 5e-1).  The gap opens at the sample length of the first stage, hw = 64 x 64 = 4096, which
       no NT list of that file has: M = 8192 (an M of test_gemm_tn's list) as two such samples, N = 8, gives 1.3e-2."""
    from tests.test_gpu_ops import NT2_CASES, close, rnd

    dt = torch.bfloat16
    # a. one product dropped from the K loop
    M, N, K, hw = 1024, 384, 1536, 1024
    assert (M, N, K, hw) in NT2_CASES
    A, Bw = rnd(M, K, dt=dt, seed=1), rnd(N, K, dt=dt, seed=2, scale=K ** -0.5)
    outs = []
    for ops in (R, drops_last_k_of_last_row()):
        C = torch.zeros(M, N, dtype=dt)
        ops.gemm("nt", A, Bw, C, M, N, K, K, K, N, dtype=dt, hw=hw)
        outs.append(C)
    assert not torch.equal(outs[0], outs[1])
    close(outs[1], outs[0], dt, "C with a dropped product")
    # b. one pixel row missing from a weight gradient
    M, N, K = 32768, 96, 128   # M of test_gemm_tn_any_split_count's rect_n_divisible case; a small N x K keeps the CPU product short
    Xo, Y = rnd(M, N, dt=dt, seed=1), rnd(M, K, dt=dt, seed=2)
    outs = []
    for ops in (R, skips_last_row_of_tn()):
        W, cs = torch.zeros(N, K), torch.zeros(N)
        ops.gemm("tn", Y, Xo, W, M, N, K, K, N, K, dtype=dt, colsum=cs)
        outs.append((W, cs))
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])
    close(outs[1][0], outs[0][0], dt, "W without its last row")
    close(outs[1][1], outs[0][1], dt, "colsum without its last row")
    # c. one row of the per-sample statistics on the neighbouring sample
    M, N, K, hw = 8192, 8, 64, 4096
    A, Bw, aux = rnd(M, K, dt=dt, seed=1), rnd(N, K, dt=dt, seed=2, scale=K ** -0.5), rnd(M, N, dt=dt, seed=5)
    outs = []
    for ops in (R, credits_last_row_of_red1_to_next_sample()):
        C, r0, r1 = torch.zeros(M, N, dtype=dt), torch.zeros(2, N), torch.zeros(2, N)
        ops.gemm("nt", A, Bw, C, M, N, K, K, K, N, dtype=dt, hw=hw, epi=R.EPI_DZ, aux=aux, ldx=N, red0=r0, red1=r1)
        outs.append(r1)
    assert not torch.equal(outs[0], outs[1])
    close(outs[1], outs[0], dt, "red1 with one row on the neighbouring sample")
