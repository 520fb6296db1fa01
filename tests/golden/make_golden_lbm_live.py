#!/usr/bin/env python3
"""Stored trace of the live LBM comparison (tests/test_lbm.py LIVE_CASES), made by RUNNING THE REFERENCE'S OWN SHADERS
(oracle/_ref/liblbm_ref.so, see make_golden_lbm.py): SHA-256 of rho, v and f after every step and of the moved tracers, written to
tests/golden/lbm_ref_live.json. Only runnable where oracle/_ref/liblbm_ref.so was built; the fixture travels with the repo."""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_lib import LbmRef
from test_lbm import LIVE_CASES, lbm_trace

out = {"x".join(map(str, dims)) + f"_{steps}": lbm_trace(LbmRef(*dims), dims, steps) for dims, steps in LIVE_CASES}
with open(os.path.join(HERE, "lbm_ref_live.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote lbm_ref_live.json", list(out))
