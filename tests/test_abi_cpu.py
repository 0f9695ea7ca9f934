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
