"""Writes tests/golden/flat_layout.json: the flat parameter layout (order, offsets, gradient buckets, sizes) of every
configuration in tests/flat_layout_cases.py, as the engines build it now.  Names and integers only; the parameter names in flat
order are stored as a SHA-256 of their newline-joined list.  Re-run only when the layout is meant to change: optimiser
checkpoints index their state by these offsets.

    python tools/gen_golden_flat_layout.py
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import flat_layout_cases as C  # noqa: E402


def _record(tag):
    core, ops = C.make(tag)
    return C.record(tag, core, core.engine(ops))


out = os.path.join(ROOT, "tests", "golden", "flat_layout.json")
with open(out, "w") as f:
    json.dump({tag: _record(tag) for tag in C.tags()}, f, separators=(",", ":"))
    f.write("\n")
print(out, os.path.getsize(out), "bytes")
