"""Writes tests/golden/engine_transcript.json: for every case of tests/engine_transcript.py, the launches of two consecutive
steps of ``viscy_amd.engine_unext2.Engine`` on the torch-stated ops (name and argument descriptions of every ops call, the
yielded bucket indices) and the zero-arena sizes after them.  The schedule on the CPU backend is fp32 with no fused pass; it
changes when a launch is added, removed, reordered or given another argument.  Re-run only when that is meant:

    python tools/gen_golden_engine_transcript.py [--package-root DIR]

``--package-root``: a directory holding another commit's ``viscy_amd/`` (a git worktree of the parent), put on the path in
front of this tree, so that the golden of a refactor comes from the commit before it while the recorder comes from this one.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "engine_transcript.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
if args.package_root:
    sys.path.insert(0, os.path.abspath(args.package_root))
import viscy_amd  # noqa: E402

if args.package_root:
    sys.path.pop(0)  # only the package comes from there: tests/ is this tree's
from tests import engine_transcript as T  # noqa: E402

print("engine from", os.path.dirname(viscy_amd.__file__))
rec = {tag: T.run_case(tag) for tag in T.CASES}
with open(args.out, "w") as f:
    json.dump(T.pack(rec), f, separators=(",", ":"))
    f.write("\n")
for tag, r in rec.items():
    print(f"{tag:32s} launches {[len(s) for s in r['steps']]}")
print(args.out, os.path.getsize(args.out), "bytes")
