#!/usr/bin/env python3
"""Generate tests/golden/restatement_ref.json by RUNNING THE REFERENCE ITSELF (oracle/_ref/soil_ref, see make_golden.py) on the cases of
tests/test_oracle_vs_ref.py: the state at tick 0 and at the last tick of every case, stored as snapshot_hashes (tests/common.py).
The odd maps of tests/oddmaps.py come twice: from the initial terrain (--sizex / --sizey), and continued from the wet start state of
that module (--load), which is the regime the device tests judge by.

Only runnable where oracle/_ref/soil_ref was built; the fixture travels with the repo."""
import json, os, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oddmaps as om
from common import (RESTATEMENT_CASES, RESTATEMENT_ODD_CASES, SOILS, restatement_case_id, restatement_odd_case_id, restatement_wet_case_id,
                    snapshot_hashes)
from oracle_lib import run_ref
from soilmachine_amd.snapshot import read_snapshot


def main():
    out = {}
    for soil, size, seed, ticks, nwater, nwind in RESTATEMENT_CASES:
        with tempfile.TemporaryDirectory() as td:
            run_ref(os.path.join(SOILS, soil), seed=seed, size=size, ticks=ticks, nwater=nwater, nwind=nwind,
                    wind=nwind > 0, dump_prefix=os.path.join(td, "r"), dump_at=[0, ticks])
            out[restatement_case_id(soil, size, seed, ticks, nwater, nwind)] = {
                "t0": snapshot_hashes(read_snapshot(os.path.join(td, "r.t0.snap"))),
                "end": snapshot_hashes(read_snapshot(os.path.join(td, f"r.t{ticks}.snap")))}
    for soil, dx, dy, seed, ticks, nwater, nwind in RESTATEMENT_ODD_CASES:
        with tempfile.TemporaryDirectory() as td:
            run_ref(os.path.join(SOILS, soil), seed=seed, sizex=dx, sizey=dy, ticks=ticks, nwater=nwater, nwind=nwind,
                    wind=nwind > 0, dump_prefix=os.path.join(td, "r"), dump_at=[0, ticks])
            out[restatement_odd_case_id(soil, dx, dy, seed, ticks, nwater, nwind)] = {
                "t0": snapshot_hashes(read_snapshot(os.path.join(td, "r.t0.snap"))),
                "end": snapshot_hashes(read_snapshot(os.path.join(td, f"r.t{ticks}.snap")))}
    for workload, (soil, nwater, nwind, wind) in om.WORKLOADS.items():
        for shape in om.SHAPES:
            with tempfile.TemporaryDirectory() as td:
                out[restatement_wet_case_id(workload, shape)] = {"t0": snapshot_hashes(om.start(workload, shape)),
                                                                 "end": snapshot_hashes(om.ref_run(workload, shape, td))}
    with open(os.path.join(HERE, "restatement_ref.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote restatement_ref.json", len(out), "cases")


if __name__ == "__main__":
    main()
