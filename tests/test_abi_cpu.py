"""CPU: the C-ABI shared library loads and exports every symbol include/vsx.h declares (no compute calls
without a GPU), the ctypes binding covers exactly those symbols, and the product path fails loudly on CPU."""

import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "vsx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vsx_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from viscy_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run `python -m viscy_amd.build`"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/vsx.h but not exported by libvsx.so"
    assert sorted(_lib.exported_symbols()) == syms  # binding and header agree
    assert _lib.lib().vsx_version() >= 1
    assert _lib.lib().vsx_get_flag(b"tn_tr") == 1
    # streaming (non-temporal) accesses are ON since round 3: their stores are compiler builtins, not the inline asm of round 1
    # (DESIGN §3 item 8); the soak / determinism tests run with the shipped values
    if not os.environ.get("VSX_FLAGS"):
        assert [_lib.lib().vsx_get_flag(f) for f in (b"nt_stream", b"grn_stream", b"ln_stream")] == [3, 2, 3]
    src = open(os.path.join(ROOT, "viscy_amd", "csrc", "vsx_common.h")).read()
    assert "global_store_dwordx4" not in src.split("__device__ __forceinline__ void stvec_stream")[1].split("ldvec_stream")[0]
    assert _lib.lib().vsx_set_flag(b"nope", 1) != 0
    assert b"unknown flag" in _lib.lib().vsx_last_error()


def test_struct_layout_matches_header():
    """VsxGemm and VsxGemmPlan are passed by pointer: field count / order of the ctypes mirrors must track the header."""
    from viscy_amd import _lib

    src = open(os.path.join(ROOT, "include", "vsx.h")).read()
    for struct in ("VsxGemm", "VsxGemmPlan"):
        head = "typedef struct %s {" % struct
        body = src[src.index(head) + len(head) : src.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl or decl.startswith("typedef"):
                continue
            for part in decl.split(","):
                m = re.search(r"(\w+)\s*(\[\d+\])?\s*$", part.strip())
                names.append(m.group(1))
        assert names == [f[0] for f in getattr(_lib, struct)._fields_], struct


# ------------------------------------------------------------------------------------------------ the binding is derived from the header
def _known_signatures():
    """rows of the table viscy_amd/_lib.py held by hand before it read the header; together they use every type word of vsx.h"""
    from viscy_amd._lib import VsxGemm, VsxGemmPlan, VsxWTask

    C = ctypes
    _I32, _F32, _P, _I64 = C.c_int32, C.c_float, C.c_void_p, C.c_int64
    return {
        "vsx_last_error": (C.c_char_p, []),
        "vsx_set_flag": (_I32, [C.c_char_p, _I32]),
        "vsx_gemm_plan": (_I32, [_I32, C.POINTER(VsxGemm), _I32, C.POINTER(VsxGemmPlan)]),
        "vsx_weight_tasks": (_I32, [C.POINTER(VsxWTask), _I32, _P]),  # was _P: typed since ops.flush hands over the array itself
        "vsx_ln_fwd": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _F32, _I32, _P]),
        "vsx_mlp_det_floats": (_I64, [_I32, _I32, _I64, _I32]),
        "vsx_spotlight_fwd": (_I32, [_P, _I32, _P, _P, _I32, _P, _I64, _I64, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P]),
        "vsx_logreg_rows": (_I32, [_P, _I64, _I32, _P, C.c_double, _P, _I32, C.c_double, C.c_double] + [_P] * 6 + [_I64, _P]),
        "vsx_row_select": (_I32, [_P, _P, _P, _I64, _I64, _I64, C.POINTER(_I64), _I32, _P]),
        "vsx_mmd_sums": (_I32, [_P, _P, _P, _I32, _I32, _I32, C.c_double, _P, _P, _I64, _P]),
    }


def _kind(t):
    """a pointer to a scalar and a void pointer marshal alike; a char pointer, a struct pointer and every scalar stand for themselves"""
    if isinstance(t, type) and issubclass(t, ctypes._Pointer) and not issubclass(t._type_, ctypes.Structure):
        return ctypes.c_void_p
    return t


def test_parser_known_answers():
    from viscy_amd import _lib

    assert _kind(ctypes.POINTER(ctypes.c_int64)) is ctypes.c_void_p and _kind(ctypes.c_char_p) is ctypes.c_char_p
    assert _kind(ctypes.POINTER(_lib.VsxGemm)) is ctypes.POINTER(_lib.VsxGemm) and _kind(ctypes.c_int64) is ctypes.c_int64
    for name, (res, args) in _known_signatures().items():
        got_res, got_args = _lib._SIGS[name]
        assert got_res is res, name
        assert [_kind(t) for t in got_args] == [_kind(t) for t in args], name
    fn = _lib.lib().vsx_spotlight_fwd   # what the loaded library's functions carry is the table
    assert (fn.restype, list(fn.argtypes)) == _lib._SIGS["vsx_spotlight_fwd"]


def _host_cc():
    import shutil

    cc = shutil.which("cc") or "/opt/rocm/llvm/bin/clang"
    assert os.path.exists(cc), "no host C compiler: neither cc nor /opt/rocm/llvm/bin/clang"
    return cc


def test_struct_layout_against_the_compiler(tmp_path):
    """size, and offset and size of every field, of the three ctypes mirrors against what the C compiler lays out from vsx.h"""
    import subprocess

    from viscy_amd import _lib

    structs = (_lib.VsxGemm, _lib.VsxGemmPlan, _lib.VsxWTask)
    assert [len(s._fields_) for s in structs] == [35, 14, 14]
    lines = ["#include <stdio.h>", '#include "vsx.h"', "int main(void) {"]
    for s in structs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (s.__name__, s.__name__))
        for f, _ in s._fields_:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s.__name__, f, s.__name__, f, s.__name__, f))
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_cc(), "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    want = []
    for s in structs:
        want.append("%s %d" % (s.__name__, ctypes.sizeof(s)))
        want += ["%s.%s %d %d" % (s.__name__, f, getattr(s, f).offset, getattr(s, f).size) for f, _ in s._fields_]
    assert out == want + [""]
    assert _lib.VsxGemmPlan.family.offset == 0 and dict(_lib.VsxGemmPlan._fields_)["family"] is ctypes.c_char_p
    assert dict(_lib.VsxGemm._fields_)["a_coff"] is ctypes.c_int32 * 8 and dict(_lib.VsxGemm._fields_)["A"] is ctypes.c_void_p


_MINI_HEADER = """/* a header in the dialect of vsx.h */
#ifdef __cplusplus
extern "C" {
#endif
typedef void* vsx_stream_t;
#define VSX_TWO 2 /* a constant */
typedef struct VsxGemm { const void* A; int32_t M, tile[2]; } VsxGemm;
%s
#ifdef __cplusplus
}
#endif
"""


def test_parser_refuses_what_it_does_not_know(monkeypatch):
    from viscy_amd import _lib

    class VsxGemm(ctypes.Structure):
        pass

    def parse(decl):
        return _lib.parse_header(_MINI_HEADER % decl, {"VsxGemm": VsxGemm})

    consts, fields, sigs = parse("int64_t vsx_ok(const VsxGemm* p, const char* s,\n    double x, vsx_stream_t stream);\nint32_t vsx_none(void);")
    assert consts == {"TWO": 2}
    assert fields == {"VsxGemm": [("A", ctypes.c_void_p), ("M", ctypes.c_int32), ("tile", ctypes.c_int32 * 2)]}
    assert sigs == {"vsx_ok": (ctypes.c_int64, [ctypes.POINTER(VsxGemm), ctypes.c_char_p, ctypes.c_double, ctypes.c_void_p]),
                    "vsx_none": (ctypes.c_int32, [])}
    for bad, named in (
        ("int32_t vsx_bad(uint16_t x, vsx_stream_t stream);", "uint16_t"),          # an unknown scalar
        ("int32_t vsx_bad(const uint16_t* x);", "uint16_t"),                        # ... behind a pointer
        ("uint16_t vsx_bad(int32_t x);", "uint16_t"),                               # ... returned
        ("int32_t vsx_bad(const VsxOther* p);", "VsxOther"),                        # a struct without a mirror class
        ("int32_t vsx_bad(float** x);", "float"),                                   # a pointer to a pointer
        ("int32_t vsx_bad(int32_t, int32_t b);", "vsx_bad"),                        # a parameter without a name
        ("int32_t vsx_bad(int32_t a, int32_t b;", "vsx_bad"),                       # a prototype that does not close
        ("int32_t vsx_bad int32_t a);", "vsx_bad"),                                 # ... or open
        ("typedef struct VsxOther { int32_t a; } VsxOther;", "VsxOther"),           # a struct without a mirror class
        ("#define VSX_SHIFTED (1 << 3)", "VSX_SHIFTED"),                            # a constant that is not a plain integer
    ):
        with pytest.raises(ValueError, match=named) as e:
            parse(bad)
        assert "vsx.h" in str(e.value), bad
    with pytest.raises(ValueError, match="VsxGemm"):   # `T* a, b` would make b a T, not a pointer
        _lib.parse_header("typedef struct VsxGemm { const void* A, B; } VsxGemm;", {"VsxGemm": VsxGemm})
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "missing.h"))
    with pytest.raises(RuntimeError, match="include/missing.h"):
        _lib._derive()


def test_constants_are_the_headers():
    from tests import ref_ops as R
    from viscy_amd import _lib, ops, reduce

    assert (_lib.VSX_F32, _lib.VSX_BF16, _lib.F32, _lib.BF16) == (0, 1, 0, 1)
    assert _lib.EPI_LN_BWD == 6 and _lib.WTASK_REDUCE_ROWS == 6 and _lib.LOSS_SLOTS == 64 and _lib.LOSS_SLOT_STRIDE == 32
    assert _lib.SPOTLIGHT_CHUNK == 16384 and _lib.NARROW_BWD_C == 5 and _lib.KNN_MAX_K == 64 and _lib.PCA_MAX_D == 4096
    assert (_lib.GEMM_NT, _lib.GEMM_TN, _lib.WTASK_MAX, _lib.SPOTLIGHT_MASK_F32, _lib.SPOTLIGHT_WS_OTSU) == (0, 1, 40, 2, 1)
    # tests/ref_ops.py states its own: the independent copy the GPU tests compute references with
    for name in ("A_ROWS", "A_PATCH2", "A_CONV3", "PRO_NONE", "PRO_GRN", "EPI_NONE", "EPI_BIAS", "EPI_BIAS_GELU_SQ", "EPI_BIAS_RES",
                 "EPI_DZ", "EPI_BIAS_STATS"):
        assert getattr(R, name) == getattr(_lib, name), name
    # the product takes the limits it checks from the header
    assert ops.KNN_MAX_K is _lib.KNN_MAX_K and ops.SPOTLIGHT_CHUNK is _lib.SPOTLIGHT_CHUNK
    assert reduce.MAX_FEATURES == _lib.PCA_MAX_D
    for f, old, new in (("online_eval.hip", "KT_MAX_K", "VSX_KNN_MAX_K"), ("pca.hip", "PCA_MAX_D", "VSX_PCA_MAX_D"),
                        ("logreg.hip", "LR_MAX_D", "VSX_PCA_MAX_D")):
        src = open(os.path.join(ROOT, "viscy_amd", "csrc", f)).read()
        assert "#define %s %s\n" % (old, new) in src, f


def test_no_cpu_fallback():
    from viscy_amd import ops
    from viscy_amd.losses import MixedLoss
    from viscy_amd.unext2 import UNeXt2

    with pytest.raises(RuntimeError, match="no CPU"):
        UNeXt2(backbone="convnextv2_atto")(torch.zeros(1, 1, 5, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU"):
        MixedLoss()(torch.zeros(1, 1, 5, 192, 192), torch.zeros(1, 1, 5, 192, 192))
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.ln_fwd(torch.zeros(4, 8), None, None, 4, 8)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "viscy_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", txt, flags=re.M), f


# every entry of the flag table in csrc/api.hip with its shipped default (bench.py writes the FLAG_NAMES ones into its JSON line)
FLAG_DEFAULTS = {
    "tn_tr": 1, "nt_wide": 1, "nt_fast": 3, "tn_wide": 1, "nt2": 17, "nt_stream": 3, "grn_stream": 2, "ggb_contig": 1,
    "tn_want": 768, "tn_p2_rounds": 1, "tn_want2": 512, "tn_fill": 1, "tn_contig": 1, "tn_stream": 3, "ln_stream": 3,
    "ggb_blocks": 2048, "tn_rect": 11, "dw_mfma": 15, "ln_fblk": 32768, "ln_bblk": 8192, "ln_ablk": 512, "ln_pack": 1,
    "mlp_fused": 111, "loss_fused": 1, "mlp_sf32": 69, "det_reduce": 0, "head_rows": 63, "head_bps": 0,
}


def test_flag_table_defaults_and_round_trip():
    import bench
    from viscy_amd import _lib

    l = _lib.lib()
    assert set(bench.FLAG_NAMES) <= set(FLAG_DEFAULTS)
    src = open(os.path.join(ROOT, "viscy_amd", "csrc", "api.hip")).read()
    assert sorted(re.findall(r'\{"(\w+)", &g_vsx_\w+, ', src)) == sorted(FLAG_DEFAULTS)  # the table and this list agree
    for name, default in FLAG_DEFAULTS.items():
        n = name.encode()
        old = l.vsx_get_flag(n)
        if not os.environ.get("VSX_FLAGS"):
            assert old == default, name
        try:
            assert l.vsx_set_flag(n, old + 1) == 0, name
            assert l.vsx_get_flag(n) == old + 1, name
        finally:
            assert l.vsx_set_flag(n, old) == 0
        assert l.vsx_get_flag(n) == old, name
    # removed with the eight-wave TN tiles
    assert l.vsx_set_flag(b"tn_want3", 256) != 0
    assert b"unknown flag 'tn_want3'" in l.vsx_last_error()
    assert l.vsx_get_flag(b"tn_want3") == -1
    # values below a flag's minimum are refused and leave it alone: the three LayerNorm caps are positive, head_bps >= 0
    for name, bad in (("ln_ablk", 0), ("ln_fblk", 0), ("ln_bblk", 0), ("ln_ablk", -1), ("head_bps", -1)):
        old = l.vsx_get_flag(name.encode())
        assert l.vsx_set_flag(name.encode(), bad) != 0, name
        assert l.vsx_get_flag(name.encode()) == old, name


# a definition or declaration of g_vsx_* ints (`int g_vsx_a = 1;`, `extern int g_vsx_a, g_vsx_b;`), not a use (`int n = g_vsx_a;`)
_FLAG_DECL = re.compile(r"^[ \t]*(?:(?:extern|static|volatile|thread_local)\s+)*int\s+g_vsx_\w+[^;(){}]*;", flags=re.M)


def test_flag_globals_are_declared_in_one_header():
    """csrc/api.hip defines the g_vsx_* ints, csrc/vsx_common.h declares them: no other .hip defines or extern-declares one"""
    csrc = os.path.join(ROOT, "viscy_amd", "csrc")
    hips = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert "api.hip" in hips and len(hips) > 10
    assert _FLAG_DECL.findall("extern int g_vsx_a;\n  int g_vsx_b = 2, g_vsx_c;\nint n = g_vsx_a;\n") == ["extern int g_vsx_a;", "  int g_vsx_b = 2, g_vsx_c;"]
    for f in hips:
        if f == "api.hip":
            continue
        src = open(os.path.join(csrc, f)).read()
        bad = _FLAG_DECL.findall(src)
        assert not bad, (f, bad)
    common = open(os.path.join(csrc, "vsx_common.h")).read()
    api = open(os.path.join(csrc, "api.hip")).read()
    defined = re.findall(r"^int (g_vsx_\w+) = ", api, flags=re.M)
    assert len(defined) == len(FLAG_DEFAULTS)
    for g in defined:
        assert re.search(r"^extern int [^;]*\b%s\b[^;]*;" % g, common, flags=re.M), g
        assert '&%s,' % g in api, g


# ------------------------------------------------------------------------------------------------ fixed-order sums: scope, sizes, scratch
def _gelu_sq_row(M, N, K, hw):
    """the fc1 launch with the GELU / sum-of-squares epilogue, as tests/gemm_plan_rows.py writes a VsxGemm (pointers only say
    which operands are there: nothing below reaches a kernel)"""
    from tests import gemm_plan_rows as G
    from tests import ref_ops as R

    return G.struct_array([dict(G.row(M, N, K, K, K, N, hw=hw), **G._epi_fields(R.EPI_BIAS_GELU_SQ, N))])[0]


def _det_plan(p):
    from viscy_amd import _lib

    plan = _lib.VsxGemmPlan()
    assert _lib.lib().vsx_gemm_plan(0, ctypes.byref(p), _lib.VSX_BF16, ctypes.byref(plan)) == 0
    return plan


def _in_thread(fn):
    import threading

    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    return out[0]


def test_det_scope_is_per_thread_and_nests():
    from viscy_amd import _lib, ops

    l = _lib.lib()
    flag0 = l.vsx_get_flag(b"det_reduce")
    l.vsx_set_flag(b"det_reduce", 0)
    p = _gelu_sq_row(1024, 384, 96, 512)

    def refused():
        """this thread's launch under det, while this thread has handed over no workspace: refused before anything is launched"""
        rc = l.vsx_gemm_nt(ctypes.byref(p), _lib.VSX_BF16, None)
        return rc, l.vsx_last_error()

    try:
        assert l.vsx_det_active() == 0
        assert l.vsx_det_scope(1) == 0
        assert l.vsx_det_active() == 1 and l.vsx_get_flag(b"det_reduce") == 0
        assert l.vsx_det_scope(1) == 1          # nested: the previous value comes back ...
        assert l.vsx_det_scope(1) == 1 and l.vsx_det_active() == 1
        assert l.vsx_det_scope(0) == 1 and l.vsx_det_active() == 0
        assert l.vsx_det_scope(1) == 0          # ... and closing hands it back
        # a thread started while this one's scope is open is outside it
        assert _in_thread(l.vsx_det_active) == 0
        assert _det_plan(p).det_floats == 1536 and _in_thread(lambda: _det_plan(p).det_floats) == 0
        # ... and its workspace is its own: handing one over there leaves this thread without
        assert l.vsx_det_workspace(None, 0) == 0
        keep = (ctypes.c_float * 1536)()
        assert _in_thread(lambda: l.vsx_det_workspace(keep, 1536)) == 0
        assert refused() == (1, b"vsx_gemm_nt: det_reduce needs vsx_det_workspace(>= 1536 floats)")
        # and one handed over here is not the other thread's, which is under its own scope there
        assert l.vsx_det_workspace(keep, 1535) == 0
        assert refused() == (1, b"vsx_gemm_nt: det_reduce needs vsx_det_workspace(>= 1536 floats)")   # one float short

        def other():
            with ops.det_scope():
                return l.vsx_det_active(), refused()

        assert _in_thread(other) == (1, (1, b"vsx_gemm_nt: det_reduce needs vsx_det_workspace(>= 1536 floats)"))
        assert l.vsx_det_scope(0) == 1 and l.vsx_det_active() == 0
        l.vsx_set_flag(b"det_reduce", 1)
        assert l.vsx_det_active() == 1 and _in_thread(l.vsx_det_active) == 1   # the flag is the process's
        with ops.det_scope():
            with ops.det_scope(False):
                assert l.vsx_det_active() == 1
        l.vsx_set_flag(b"det_reduce", 0)
        with ops.det_scope():
            assert l.vsx_det_active() == 1
            with ops.det_scope():
                pass
            assert l.vsx_det_active() == 1
        assert l.vsx_det_active() == 0
    finally:
        l.vsx_det_scope(0)
        l.vsx_det_workspace(None, 0)
        l.vsx_set_flag(b"det_reduce", flag0)


def test_det_size_queries_against_the_formulas_they_replace():
    """what viscy_amd.ops computed by hand before the library was asked: the query is never larger, and equal wherever the
    launch exists — except the GEMM, where the old formula carried a spare row: (M // 256 + 1) * N against (M / BM) * N"""
    from viscy_amd import _lib

    l = _lib.lib()
    served = 0
    for C in (64, 96, 192, 224, 384):
        for hw in (64, 100, 256, 512, 1024, 4096):
            for B in (1, 2, 3, 8):
                M = B * hw
                for mode in range(8):
                    q, old = l.vsx_mlp_det_floats(C, hw, M, mode), (M // 256) * 4 * C
                    if mode in (0, 2, 6) and l.vsx_mlp_mode_supported(C, hw, M, mode, _lib.VSX_BF16):
                        served += 1
                        assert q == old > 0, (C, hw, B, mode, q, old)
                        rows = l.vsx_mlp_rows_per_workgroup(C, hw, M)   # the geometry, as the dh passes' workspace asks for it
                        assert rows == 0 or q == M // rows * 4 * C
                    else:
                        assert q == 0, (C, hw, B, mode, q)
    assert served >= 100
    for B in (1, 2, 3):
        for H2 in (8, 16, 24, 32, 48, 2048):
            for W2 in (16, 24, 32, 64, 2048):
                q, old = l.vsx_head_conv_det_floats(B, H2, W2), B * (H2 // 8) * (W2 // 16) * 64
                if l.vsx_head_conv_supported(H2, W2, 8, 32, 5, _lib.VSX_BF16):
                    assert q == old > 0, (B, H2, W2, q, old)
                else:
                    assert q == 0, (B, H2, W2, q)
    assert l.vsx_head_conv_det_floats(0, 16, 16) == 0
    nonzero = 0
    assert l.vsx_det_scope(1) == 0
    try:
        for hw in (64, 128, 256, 512, 1024, 4096):
            for B in (1, 2, 8):
                for N, K in ((384, 96), (768, 192), (896, 224), (1536, 384), (100, 96)):
                    M = B * hw
                    p, plan = _gelu_sq_row(M, N, K, hw), _lib.VsxGemmPlan()
                    if l.vsx_gemm_plan(0, ctypes.byref(p), _lib.VSX_BF16, ctypes.byref(plan)) != 0:
                        continue
                    old = (M // 256 + 1) * N
                    assert plan.det_floats <= old
                    if plan.family == b"gemm_nt2" and hw % 256 == 0 and hw > 256:   # two or more 256-row tiles per sample
                        nonzero += 1
                        assert plan.det_floats == (M // 256) * N == old - N
                    else:
                        assert plan.det_floats == 0
    finally:
        l.vsx_det_scope(0)
    assert nonzero >= 30


def test_scratch_never_releases_and_stays_within_twice_its_largest_buffer():
    from viscy_amd import ops

    allocated = []

    def alloc(floats, dev):
        allocated.append(floats)
        return torch.empty(floats, dtype=torch.float32)

    sc = ops.Scratch(alloc)
    handed = []   # (address, floats) of every request
    for n in (10, 5, 11, 100, 100, 101, 3, 1000, 999, 2001, 1):
        t = sc.take("dev0", n)
        assert t.numel() >= n
        handed.append((t.data_ptr(), n))
    assert allocated == [10, 20, 100, 200, 1000, 2001]   # grows by appending max(request, twice the last)
    spans = [(b.data_ptr(), b.data_ptr() + 4 * b.numel()) for b in sc.held]
    assert len(sc.held) == len(allocated)
    for addr, n in handed:   # every address a launch may still hold lies in a buffer that is alive
        assert any(lo <= addr and addr + 4 * n <= hi for lo, hi in spans), (addr, n)
    assert sum(b.numel() for b in sc.held) <= 2 * max(b.numel() for b in sc.held)
    assert sc.take("dev1", 4).data_ptr() != sc.take("dev0", 4).data_ptr()   # one arena per device
    mine = sc.take("dev0", 7)
    theirs = _in_thread(lambda: sc.take("dev0", 7))   # ... and per thread
    assert theirs.data_ptr() != mine.data_ptr() and theirs.numel() == 7
    assert any(b is theirs for b in sc.held)   # kept after its thread has ended
    assert sc.take("dev0", 7) is mine
