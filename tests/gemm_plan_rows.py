"""The launches whose dispatch tests/golden/gemm_plan_table.json records: VsxGemm parameter sets as plain dicts, in a fixed order.

``groups()`` yields (kind, flags, dtype code, rows): one flag setting and dtype of one row list.  Pointer fields hold 1 where a
path needs them (nothing here is ever dereferenced: the planners only test pointers for NULL).

1. every case of ``nt_cases()`` / ``tn_cases()`` of tests/ref_exact_gemm.py, with the strides and offsets its runner passes, under
   each of its flag settings, epilogues and dtypes;
2. the real-shape grid: M = B h w for B = 512 on 64^2 .. 8^2 maps and B = 8 on 512^2 .. 64^2 maps, N and K from {C, 4C} for the five
   stage widths, plus the shapes of GEMM_CASES / NT2_CASES of tests/test_gpu_ops.py; crossed with the prologue forms, every NT
   epilogue, per-sample weights / outputs, the 2 x 2 patch gather and scatter, hw per sample or 0, both dtypes;
3. the same grid under every single-flag departure from the shipped values, for each flag the dispatch reads;
4. launches that are refused."""

from __future__ import annotations

from tests import ref_exact_gemm as X
from tests import ref_ops as R

NT, TN = 0, 1
F32, BF16 = 0, 1
PAD = X.PAD

# flag -> the values it is swept over (the shipped value is left out where the issue's list names it)
TN_SWEEP = {"tn_tr": (0,), "tn_wide": (0,), "tn_rect": (0, 1, 2, 3, 8), "tn_want": (97, 333), "tn_want2": (97, 333, 768), "tn_fill": (0,),
            "tn_contig": (0,), "tn_stream": (0, 1, 2), "tn_p2_rounds": (0, 2), "nt_fast": (0, 1)}
NT_SWEEP = {"nt_fast": (0, 1), "nt_wide": (0, 2), "nt2": (0, 1, 3, 5, 9), "nt_stream": (0, 1, 2), "det_reduce": (1,)}
SHIPPED = {"tn_tr": 1, "tn_wide": 1, "tn_rect": 11, "tn_want": 768, "tn_want2": 512, "tn_fill": 1, "tn_contig": 1, "tn_stream": 3,
           "tn_p2_rounds": 1, "nt_fast": 3, "nt_wide": 1, "nt2": 17, "nt_stream": 3, "det_reduce": 0}


def row(M, N, K, lda, ldb, ldc, **kw):
    r = dict(A=1, B=1, C=1, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, nz=1)
    r.update(kw)
    return r


def _epi_fields(epi, N):
    """the operands an NT epilogue needs"""
    f = dict(epi=epi, bias=1)
    if epi == R.EPI_BIAS_RES:
        f.update(res=1, ldr=N)
    elif epi == R.EPI_DZ:
        f.update(aux=1, ldx=N, red0=1, red1=1)
    elif epi == R.EPI_BIAS_STATS:
        f.update(red0=1, red1=1)
    elif epi == R.EPI_BIAS_GELU_SQ:
        f.update(red0=1, C2=1)
    elif epi == 6:   # EPI_LN_BWD: aux = xh, grn_s = rstd
        f.update(aux=1, ldx=N, grn_s=1)
    return f


# ------------------------------------------------------------------------------------------------ 1. the exact-test cases
def nt_case_rows(case):
    """what run_nt_case of tests/ref_exact_gemm.py passes, one row per epilogue variant"""
    M, N, K, nz = case["M"], case["N"], case["K"], case["nz"]
    if case["a_mode"] == R.A_ROWS:
        a_coff, lda = [PAD], K + 2 * PAD
    elif case["a_mode"] == R.A_PATCH2:
        a_coff, lda = [PAD], case["cs"] + 2 * PAD
    else:
        a_coff, lda = [PAD + z * case["c3"] for z in range(nz)], (nz + 2) * case["c3"] + 2 * PAD
    ldb = K + PAD
    cw = case["c_cs"] if case["c_mode"] == R.A_PATCH2 else nz * N
    base = row(M, N, K, lda, ldb, cw + 2 * PAD, nz=nz, a_coff=a_coff, b_off=[0] * nz, c_coff=[PAD + z * N for z in range(nz)],
               a_mode=case["a_mode"], c_mode=case["c_mode"], cs=case["cs"], c_cs=case["c_cs"], pro=case["pro"], hw=case["hw"])
    if case["grid"] is not None:
        base.update(gh=case["grid"][1], gw=case["grid"][2])
    if case["pro"] == R.PRO_GRN:
        base.update(grn_s=1, grn_b=1)
    if case["bstride"]:
        base.update(b_bstride=N * ldb)
    rows = []
    for name in case["epis"]:
        epi, with_bias, with_rscale = X.EPIS[name]
        r = dict(base, **_epi_fields(epi, N + PAD))
        r["bias"] = 1 if with_bias else 0
        r["rscale"] = 1 if with_rscale else 0
        rows.append(r)
    return rows


def tn_case_row(case):
    M, N, K = case["M"], case["N"], case["K"]
    r = row(M, N, K, K + 2 * PAD, N + 2 * PAD, K + 2 * PAD, a_coff=[PAD], b_off=[PAD], c_coff=[PAD], pro=case["pro"], hw=case["hw"], colsum=1)
    if case["patch"]:
        B, gh, gw, cin = case["patch"]
        r.update(lda=cin + 2 * PAD, a_mode=R.A_PATCH2, gh=gh, gw=gw, cs=cin)
    if case["pro"] == R.PRO_GRN:
        r.update(grn_s=1, grn_b=1)
    if case["per_sample"]:
        r.update(ldc=K, c_coff=[0], b_bstride=N * K)
    if case["stats"]:
        r.update(aux=1, ldx=K + PAD, red0=1)
    return r


def _case_groups():
    dcode = {X.F32: F32, X.BF16: BF16}
    for case in X.nt_cases():
        for dt in case["dts"]:
            for setting in case["flags"]:
                yield NT, dict(setting), dcode[dt], nt_case_rows(case)
    for case in X.tn_cases():
        for dt in case["dts"]:
            for setting in case["flags"]:
                for tr in (case["tr"] if dt == X.BF16 else case["tr"][:1]):
                    yield TN, dict(setting, tn_tr=tr), dcode[dt], [tn_case_row(case)]


# ------------------------------------------------------------------------------------------------ 2. the real-shape grid
def shapes():
    out = []
    for B, sides in ((512, (64, 32, 16, 8)), (8, (512, 256, 128, 64))):
        for side in sides:
            for C in (96, 192, 384, 768, 224):
                for N in (C, 4 * C):
                    for K in (C, 4 * C):
                        out.append((B * side * side, N, K, side * side, side))
    from tests.test_gpu_ops import GEMM_CASES, NT2_CASES

    for M, N, K, hw in list(GEMM_CASES) + list(NT2_CASES):
        side = int(round(hw ** 0.5))
        out.append((M, N, K, hw, side if side * side == hw and M % hw == 0 else 0))
    return out


def _pro_forms():
    return (dict(pro=R.PRO_NONE), dict(pro=R.PRO_GRN, grn_s=1, grn_b=1), dict(pro=R.PRO_GRN, grn_s=1, grn_b=1, aux=1, red0=1))


_GRID: dict = {}


def grid_rows(kind):
    if kind in _GRID:
        return _GRID[kind]
    rows = []
    for M, N, K, hw_s, side in shapes():
        for pro in _pro_forms():
            for bstride in (0, N * K):
                for a_mode in (R.A_ROWS, R.A_PATCH2):
                    if a_mode == R.A_PATCH2 and not side:
                        continue
                    gather = dict(a_mode=a_mode, gh=side, gw=side, cs=K // 4, lda=K // 4) if a_mode == R.A_PATCH2 else {}
                    for hw in (hw_s, 0):
                        if kind == TN:
                            rows.append(dict(row(M, N, K, K, N, K, hw=hw, b_bstride=bstride, colsum=1, ldx=K), **pro, **gather))
                            continue
                        for c_mode in (R.A_ROWS, R.A_PATCH2):
                            if c_mode == R.A_PATCH2 and not side:
                                continue
                            scatter = dict(c_mode=c_mode, c_cs=N // 4, ldc=N // 4, gh=side, gw=side) if c_mode == R.A_PATCH2 else {}
                            for epi in range(7):
                                r = dict(row(M, N, K, K, K, N, hw=hw, b_bstride=bstride), **gather)
                                r.update(_epi_fields(epi, N))
                                r.update(pro)   # (the third prologue form sets aux / red0 whatever the epilogue)
                                r.update(scatter)
                                rows.append(r)
    _GRID[kind] = rows
    return rows


def _grid_groups():
    for kind, sweep in ((TN, TN_SWEEP), (NT, NT_SWEEP)):
        settings = [{}] + [{f: v} for f, vals in sweep.items() for v in vals]
        for setting in settings:
            for dt in (BF16, F32):
                yield kind, setting, dt, grid_rows(kind)


# ------------------------------------------------------------------------------------------------ 4. refused launches
def refused_groups():
    ok = row(512, 128, 96, 96, 96, 128, hw=256)
    tn_ok = row(1024, 96, 384, 384, 96, 384, hw=64, colsum=1)
    stats = dict(tn_ok, pro=R.PRO_GRN, grn_s=1, grn_b=1, aux=1, ldx=384, red0=1)
    nt_bad = [dict(ok, N=100), dict(ok, K=100), dict(ok, lda=100), dict(ok, ldc=132), dict(ok, M=0), dict(ok, nz=9), dict(ok, a_coff=[4]),
              dict(ok, a_mode=R.A_PATCH2, gh=0, gw=16, cs=24), dict(ok, a_mode=R.A_PATCH2, gh=16, gw=16, cs=40),
              dict(ok, a_mode=R.A_PATCH2, gh=16, gw=12, cs=24), dict(ok, c_mode=R.A_PATCH2, c_cs=0, gh=16, gw=16),
              dict(ok, pro=R.PRO_GRN), dict(ok, pro=R.PRO_GRN, grn_s=1, grn_b=1, hw=0),
              dict(ok, epi=R.EPI_DZ), dict(ok, epi=R.EPI_DZ, red0=1, hw=256), dict(ok, epi=R.EPI_BIAS_GELU_SQ, red0=1),
              dict(ok, epi=R.EPI_BIAS_STATS, red0=1), dict(ok, epi=R.EPI_BIAS_RES), dict(ok, rscale=1), dict(ok, epi=R.EPI_BIAS_RES, res=1, rscale=1, hw=0),
              dict(ok, epi=6, aux=1, grn_s=1, N=512, ldc=512), dict(ok, epi=6, aux=1), dict(ok, epi=6, aux=1, grn_s=1, M=520),
              dict(ok, b_bstride=128 * 96, hw=100), dict(ok, b_bstride=128 * 96, N=64, ldc=64), dict(ok, b_bstride=128 * 96, K=104, lda=104, ldb=104)]
    tn_bad = [dict(tn_ok, epi=R.EPI_BIAS), dict(tn_ok, c_mode=R.A_PATCH2), dict(tn_ok, N=100), dict(tn_ok, ldb=100),
              dict(tn_ok, b_bstride=96 * 384, hw=100), dict(tn_ok, b_bstride=96 * 384, hw=0), dict(tn_ok, b_bstride=96 * 384, nz=2),
              dict(tn_ok, b_bstride=96 * 384, pro=R.PRO_GRN, grn_s=1, grn_b=1), dict(tn_ok, b_bstride=96 * 384, M=1000),
              dict(stats, hw=100), dict(stats, hw=32), dict(stats, N=64, ldb=64), dict(stats, K=96, lda=96, ldc=96), dict(stats, ldx=376),
              dict(stats, M=1000), dict(stats, nz=2), dict(stats, a_mode=R.A_PATCH2, gh=8, gw=8, cs=96, lda=96)]
    for dt in (BF16, F32, 2):
        yield NT, {}, dt, nt_bad
        yield TN, {}, dt, tn_bad
    yield TN, {"tn_tr": 0}, BF16, [stats, dict(tn_ok, b_bstride=96 * 384)]
    yield TN, {"nt_fast": 0}, BF16, [stats, dict(tn_ok, b_bstride=96 * 384)]
    yield NT, {"nt_fast": 0}, BF16, [dict(ok, b_bstride=128 * 96)]


def _extra_groups():
    """instantiations the rows above do not reach: bf16 128-tiles with scalar LDS reads and 32-row steps (M % 64 != 0)"""
    r = row(4128, 384, 1024, 1024, 384, 1024, colsum=1)
    yield TN, {"tn_tr": 0}, BF16, [r, dict(r, pro=R.PRO_GRN, grn_s=1, grn_b=1, hw=32)]


def groups():
    yield from _case_groups()
    yield from _grid_groups()
    yield from refused_groups()
    yield from _extra_groups()


# ------------------------------------------------------------------------------------------------ walking the rows
FIELDS = ("rc", "text", "esize", "tile0", "tile1", "step", "nbuf", "pro_kind", "tr", "epi", "grid0", "grid1", "grid2", "block", "pro_bits",
          "zero_c", "zero_colsum", "det_floats")   # one outcome; `text` indexes the table's strings: the family, or the error of a refusal

_ARRAYS: dict = {}


def struct_array(rows):
    """the rows as a ctypes array of VsxGemm (kept per row list: the grid is walked once per flag setting)"""
    from viscy_amd._lib import VsxGemm

    if id(rows) not in _ARRAYS:
        arr = (VsxGemm * len(rows))()
        for p, r in zip(arr, rows):
            for k, v in r.items():
                if isinstance(v, list):
                    a = getattr(p, k)
                    for i, x in enumerate(v):
                        a[i] = x
                elif v:
                    setattr(p, k, v)
        _ARRAYS[id(rows)] = (rows, arr)
    return _ARRAYS[id(rows)][1]


def walk_plans(lib):
    """every row through vsx_gemm_plan: (outcomes [rows, len(FIELDS)] with ``text`` indexing the returned strings, strings)"""
    import ctypes as C

    import numpy as np

    from viscy_amd._lib import VsxGemm, VsxGemmPlan

    plan = C.cast(lib.vsx_gemm_plan, C.CFUNCTYPE(C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p))
    dt_plan = np.dtype([("family", "u8"), ("i", "i4", 13), ("z", "i8", 3)], align=True)
    assert dt_plan.itemsize == C.sizeof(VsxGemmPlan)
    strings, index, out = [], {}, []

    def sid(b):
        if b not in index:
            index[b] = len(strings)
            strings.append(b.decode())
        return index[b]

    fam_ids = {}
    for kind, setting, dt, rows in groups():
        arr, n = struct_array(rows), len(rows)
        plans = (VsxGemmPlan * n)()
        a0, p0, sa, sp = C.addressof(arr), C.addressof(plans), C.sizeof(VsxGemm), C.sizeof(VsxGemmPlan)
        saved = {f: lib.vsx_get_flag(f.encode()) for f in setting}
        res = np.zeros((n, len(FIELDS)), dtype=np.int64)
        try:
            for f, v in setting.items():
                assert lib.vsx_set_flag(f.encode(), v) == 0, f
            for i in range(n):
                rc = plan(kind, a0 + i * sa, dt, p0 + i * sp)
                if rc:
                    res[i, 0], res[i, 1] = rc, sid(lib.vsx_last_error())
        finally:
            for f, v in saved.items():
                lib.vsx_set_flag(f.encode(), v)
        got = np.frombuffer(plans, dtype=dt_plan)
        good = res[:, 0] == 0
        for ptr in np.unique(got["family"][good]):
            if int(ptr) not in fam_ids:
                fam_ids[int(ptr)] = sid(C.string_at(int(ptr)))
        res[good, 1] = [fam_ids[int(x)] for x in got["family"][good]]
        res[good, 2:15] = got["i"][good]
        res[good, 15:18] = got["z"][good]
        out.append(res)
    return np.concatenate(out), strings
