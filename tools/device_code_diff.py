#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, object by object (CPU only; no GPU work).

    python -m viscy_amd.build                                             # this tree  -> viscy_amd/_build
    VSX_CSRC=<csrc of the other commit> python -m viscy_amd.build parent  # the other  -> viscy_amd/_build_parent
    python tools/device_code_diff.py viscy_amd/_build viscy_amd/_build_parent

A host-only change must leave every kernel as it was.  For every .o the device code object is extracted with
`llvm-objdump --offloading`; two objects are equal when their `llvm-objdump -d` text and the (name, type, size) rows of
their `llvm-readelf -s` symbol tables agree (`__hip_cuid_*`, a hash of the source text, is left out).  One line per
object, exit status 1 on any difference or on an object that only one side has.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(tool: str, *args: str, cwd: str | None = None) -> str:
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def device_code(obj: str, tmp: str) -> tuple[list[str], list[tuple[str, str, str]]]:
    """(disassembly lines, sorted symbol rows) of the gfx950 code object bundled in `obj`"""
    shutil.copy(obj, os.path.join(tmp, "o"))  # the bundles are written next to the input, under its name
    run("llvm-objdump", "--offloading", "o", cwd=tmp)
    co = [f for f in os.listdir(tmp) if "amdgcn" in f and f.endswith("gfx950")]
    if not co:  # a file without kernels (api.hip) bundles no device code
        return [], []
    if len(co) != 1:
        raise RuntimeError(f"{obj}: expected one gfx950 code object, found {co}")
    path = os.path.join(tmp, co[0])
    text = [line for line in run("llvm-objdump", "-d", path).splitlines() if "file format" not in line]  # drop the path line
    syms = []
    for line in run("llvm-readelf", "-s", "-W", path).splitlines():
        f = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(f) >= 8 and f[0].rstrip(":").isdigit() and not f[7].startswith("__hip_cuid_"):
            syms.append((f[7], f[3], f[2]))
    return text, sorted(set(syms))  # .dynsym and .symtab list the same functions


def main(a: str, b: str) -> int:
    names = sorted({f for d in (a, b) for f in os.listdir(d) if f.endswith(".o")})
    bad = kernels = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{n:22s} MISSING in {b if os.path.exists(pa) else a}")
            bad += 1
            continue
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            (ta_text, ta_syms), (tb_text, tb_syms) = device_code(pa, ta), device_code(pb, tb)
        nk = sum(1 for s in ta_syms if s[1] == "FUNC")
        kernels += nk
        why = [w for w, same in (("disassembly", ta_text == tb_text), ("symbols", ta_syms == tb_syms)) if not same]
        if "symbols" in why:
            why.append("only one side: " + " ".join(sorted(s[0] for s in set(ta_syms) ^ set(tb_syms))[:6]))
        print(f"{n:22s} {'DIFFERENT: ' + ', '.join(why) if why else 'equal'}  ({nk} functions, {len(ta_text)} lines)")
        bad += bool(why)
    print(f"{len(names)} objects, {kernels} functions: {'all equal' if not bad else f'{bad} DIFFERENT'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
