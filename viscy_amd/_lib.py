"""ctypes binding of libvsx.so, derived at import from the C-ABI's one statement, include/vsx.h: the signatures, the three
structs and the VSX_* constants are what the header says.

There is NO fallback: if the shared library is missing or a tensor is not on a HIP device the
wrappers raise — a silent eager-PyTorch path would void every parity / performance claim.
"""

from __future__ import annotations

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VSX_LIB", os.path.join(_HERE, "libvsx.so"))  # VSX_LIB: A/B-test another build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vsx.h")

# the type words of the header, and what a pointer to one becomes: buffers are opaque addresses, a char pointer is a C string
_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_POINTERS = dict.fromkeys(("void", "float", "double", "int32_t", "int64_t", "uint8_t", "uint64_t"), C.c_void_p) | {"char": C.c_char_p}


def parse_header(text: str, structs: dict[str, type]) -> tuple[dict, dict, dict]:
    """The subset of C that include/vsx.h is written in -> (constants {NAME: value} of `#define VSX_NAME <integer>`,
    fields {struct: its _fields_}, signatures {vsx_name: (restype, argtypes)}).  ``structs``: the mirror class of every struct of
    the header; a pointer to one is typed.  There is no default type: anything else raises ValueError with the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+VSX_(\w+)[ \t]+(\S[^\n]*)$", text, flags=re.M):
        try:
            consts[m[1]] = int(m[2], 0)
        except ValueError:
            raise ValueError(f"vsx.h: VSX_{m[1]} is not an integer constant: {m[2].strip()}") from None
    # as a C compiler reads it: no macro is defined, so every #ifdef block (extern "C") goes, then the other directives
    text = re.sub(r"^[ \t]*#[ \t]*ifdef\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", "", text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    types = dict(_SCALARS)

    def ctype(spec: str, where: str):
        words = [w for w in spec.replace("*", " * ").split() if w != "const"]
        if len(words) == 1 and words[0] in types:
            return types[words[0]]
        if len(words) == 2 and words[1] == "*":
            if words[0] in structs:
                return C.POINTER(structs[words[0]])
            if words[0] in _POINTERS:
                return _POINTERS[words[0]]
        raise ValueError(f"vsx.h: unknown type '{' '.join(spec.split())}' in: {where}")

    def declare(decl: str, where: str) -> list:
        """one declaration, `const float* x` or `int32_t grid[3], block` -> [(name, ctype), ...]"""
        out, spec = [], ""
        for d in decl.split(","):
            m = re.fullmatch(r"(.*[\s*])?(\w+)\s*(?:\[(\d+)\])?", d.strip(), flags=re.S)
            spec = (m and m[1] or "").strip() or spec
            if not m or not spec or (out and "*" in spec):  # (`T* a, b` declares b a T: write one pointer per declaration)
                raise ValueError(f"vsx.h: cannot read '{' '.join(d.split())}' in: {where}")
            t = ctype(spec, where)
            out.append((m[2], t * int(m[3]) if m[3] else t))
        return out

    fields = {}

    def struct(m: re.Match) -> str:
        if m[1] != m[3] or m[1] not in structs:
            raise ValueError(f"vsx.h: struct {m[1]} / {m[3]} has no mirror class")
        fields[m[1]] = [f for decl in m[2].split(";") if decl.strip() for f in declare(decl, "struct " + m[1])]
        return ""

    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    sigs = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        if m := re.fullmatch(r"typedef (.+?)(\w+)", stmt):
            types[m[2]] = ctype(m[1], stmt)
        elif m := re.fullmatch(r"(.+?)\b(vsx_\w+) ?\((.*)\)", stmt):
            args = [] if m[3].strip() == "void" else [t for p in m[3].split(",") for _, t in declare(p, stmt)]
            sigs[m[2]] = (ctype(m[1], stmt), args)
        else:
            raise ValueError(f"vsx.h: neither a typedef nor a prototype: {stmt}")
    return consts, fields, sigs


class VsxGemm(C.Structure):
    """one vsx_gemm_nt / vsx_gemm_tn launch (include/vsx.h)"""


class VsxGemmPlan(C.Structure):
    """what vsx_gemm_plan answers (include/vsx.h)"""


class VsxWTask(C.Structure):
    """one job of vsx_weight_tasks (include/vsx.h)"""


def _derive() -> dict:
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"viscy_amd: {HEADER_PATH} not found — the ctypes binding is derived from this header")
    structs = {c.__name__: c for c in (VsxGemm, VsxGemmPlan, VsxWTask)}
    with open(HEADER_PATH) as f:
        consts, fields, sigs = parse_header(f.read(), structs)
    for name, cls in structs.items():
        cls._fields_ = fields[name]
    # VSX_EPI_BIAS of the header is EPI_BIAS here; the two dtype codes keep their prefixed names as well
    globals().update(consts, VSX_F32=consts["F32"], VSX_BF16=consts["BF16"])
    return sigs


_SIGS = _derive()
_lib = None


def exported_symbols() -> list[str]:
    return sorted(_SIGS)


def lib() -> C.CDLL:
    """Load libvsx.so (once). Raises if it has not been built: `python -m viscy_amd.build`."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"viscy_amd: {LIB_PATH} not found — the HIP kernels are mandatory (no CPU / eager fallback). "
                "Build them with `python -m viscy_amd.build` (hipcc, --offload-arch=gfx950)."
            )
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)  # AttributeError here = header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = l
        # VSX_FLAGS="nt2=0,tn_rect=0": tuning knobs of vsx_set_flag for A/B runs of unmodified programs (bench.py, tests)
        for kv in filter(None, os.environ.get("VSX_FLAGS", "").split(",")):
            name, _, val = kv.partition("=")
            if l.vsx_set_flag(name.strip().encode(), int(val)) != 0:
                raise RuntimeError(f"VSX_FLAGS: {l.vsx_last_error().decode(errors='replace')}")
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().vsx_last_error().decode(errors="replace")
        raise RuntimeError(f"libvsx {what} failed (rc={rc}): {msg}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return VSX_F32
    if dt == torch.bfloat16:
        return VSX_BF16
    raise TypeError(f"viscy_amd kernels compute in float32 or bfloat16, got {dt}")


def ptr(t: torch.Tensor | None) -> int | None:
    """Device pointer of a contiguous HIP tensor (None → NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("viscy_amd: tensor is not on a HIP device — the MI355X kernels have no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("viscy_amd: tensor must be contiguous")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream
