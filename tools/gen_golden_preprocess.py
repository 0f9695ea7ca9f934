"""Writes tests/golden/preprocess_stats.json: what the reference's get_val_stats (viscy_utils/mp_utils.py, which imports only numpy)
gives on the seeded arrays of tests/ref_preprocess.golden_cases().

    python tools/gen_golden_preprocess.py <reference checkout>/packages/viscy-utils/src/viscy_utils

mp_utils.py is loaded by file path.  Results only, no inputs: the arrays are rebuilt from their seed.  Every value is written as
``float.hex()``, so the file holds the bits.  The rest of the reference's preprocess (generate_normalization_metadata,
generate_fg_masks) needs iohub, tensorstore and scikit-image and is not recorded.
  numpy              the numpy version the values were taken with (percentile interpolation and float32 means are numpy's)
  stats[name][key]   get_val_stats(case)[key]
  keys               the order of the keys"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_preprocess as RP  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("reference_mp_utils", os.path.join(sys.argv[1], "mp_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stats, keys = {}, None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, arr in RP.golden_cases().items():
            row = mod.get_val_stats(arr)
            assert all(type(v) is float for v in row.values())
            keys = list(row)
            stats[name] = {k: v.hex() for k, v in row.items()}
    out = os.path.join(ROOT, "tests", "golden", "preprocess_stats.json")
    with open(out, "w") as f:
        json.dump({"numpy": np.__version__, "keys": keys, "stats": stats}, f, indent=1)
    print(out)


if __name__ == "__main__":
    main()
