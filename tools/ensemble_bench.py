#!/usr/bin/env python3
"""Ensembles of exact maps (smx_ensemble_*): the tick of B members against one standalone SERIAL context and the reference's
one-core loop. Workload: default.soil at 256^2, 250 water + 250 wind particles per tick, seeds 0..B-1, pools of 8 sections per
cell; 5 warm-up ticks, 20 timed. Prints one JSON line and writes profiles/r07_ensemble_<tag>.json.

usage: ensemble_bench.py [--batches 1,8,64,256,1024] [--warmup 5] [--ticks 20] [--tag bench] [--out profiles] [--no-record] [--no-ref]

Per B: ms per ensemble tick from device events (and its phase split), wall ms per tick, aggregate top-level water steps per second,
per-member slowdown against B = 1. Next to it: the same ticks on one standalone SERIAL context, and the reference's own loop
(oracle/_ref/soil_ref_lean, run as tools/p2_reference.py runs it, one process per core) for one member: from that, how many host
cores the ensemble is worth."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soilmachine_amd import capi                       # noqa: E402
from soilmachine_amd.ensemble import Ensemble          # noqa: E402
from soilmachine_amd.machine import Layermap           # noqa: E402
from soilmachine_amd.soilfile import loadsoil          # noqa: E402

SOIL, SIZE, NWATER, NWIND = "default.soil", 256, 250, 250
PHASES = ("ms_water", "ms_grid", "ms_wind", "ms_freq")


def _tick_ms(t: dict) -> float:
    return sum(t[k] for k in PHASES)


def run_ensemble(cfg, b: int, warmup: int, ticks: int) -> dict:
    pool = 8 * SIZE * SIZE
    t0 = time.perf_counter()
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, SIZE, SIZE, seed=s, pool=pool) for s in range(b)]
        t_add = time.perf_counter() - t0
        ens.tick(NWATER, NWIND, n=warmup)
        ens.sync()
        s0 = sum(m.counters()["steps_water_top"] for m in mem)
        ens.timing_reset()
        w0 = time.perf_counter()
        ens.tick(NWATER, NWIND, n=ticks)
        ens.sync()
        wall = time.perf_counter() - w0
        t = ens.timing()
        cs = [m.counters() for m in mem]
    steps = sum(c["steps_water_top"] for c in cs) - s0
    dev_ms = _tick_ms(t) / ticks
    return {"members": b, "ms_per_tick": round(dev_ms, 3), "wall_ms_per_tick": round(1e3 * wall / ticks, 3),
            "phase_ms_per_tick": {k[3:]: round(t[k] / ticks, 3) for k in PHASES},
            "kernel_ms_per_tick": {k: round(t["ms_kernel_" + k] / ticks, 3) for k in ("water", "wind", "classify", "mapfreq")},
            "launches_per_tick": {k: t["launches_" + k] / ticks for k in ("kernel_water", "kernel_wind", "kernel_classify", "kernel_mapfreq")},
            "water_steps_top": steps, "water_steps_per_s": round(steps / (dev_ms * ticks / 1e3), 1),
            "pool_overflow": sum(c["pool_overflow"] for c in cs), "s_to_add_members": round(t_add, 2)}


def run_standalone(cfg, warmup: int, ticks: int) -> dict:
    m = Layermap(cfg, SIZE, SIZE, seed=0, pool=8 * SIZE * SIZE, engine=capi.ENGINE_SERIAL)
    for _ in range(warmup):
        m._chk(m.L.smx_tick(m.h, NWATER, NWIND, 1, 1))
    m.sync()
    s0 = m.counters()["steps_water_top"]
    m.timing_reset()
    w0 = time.perf_counter()
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, NWATER, NWIND, 1, 1))
    m.sync()
    wall = time.perf_counter() - w0
    t = m.timing()
    steps = m.counters()["steps_water_top"] - s0
    m.close()
    dev_ms = _tick_ms(t) / ticks
    return {"ms_per_tick": round(dev_ms, 3), "wall_ms_per_tick": round(1e3 * wall / ticks, 3),
            "phase_ms_per_tick": {k[3:]: round(t[k] / ticks, 3) for k in PHASES}, "water_steps_top": steps}


def run_reference(warmup: int, ticks: int) -> dict:
    """soil_ref_lean for warmup and for warmup + ticks ticks (two processes on two cores): the difference of the phase times is the
    reference's own time for the timed ticks of one member."""
    exe = os.path.join(ROOT, "oracle", "_ref", "soil_ref_lean")
    if not os.path.exists(exe):
        return {"skipped": "oracle/_ref/soil_ref_lean is not built (oracle/Makefile needs the reference tree)"}
    procs = []
    with tempfile.TemporaryDirectory() as td:
        for k, n in enumerate((warmup, warmup + ticks)):
            cmd = [exe, "--soil", os.path.join(ROOT, "soilmachine_amd", "soils", SOIL), "--seed", "0", "--size", str(SIZE), "--ticks", str(n),
                   "--nwater", str(NWATER), "--nwind", str(NWIND), "--wind", "1", "--pool", str(8 * SIZE * SIZE),
                   "--heights-out", os.path.join(td, f"h{k}.bin")]
            procs.append(subprocess.Popen(["taskset", "-c", str(k + 1)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True))
        outs = [p.communicate()[0] for p in procs]
    js = []
    for out in outs:
        j = next((json.loads(line[5:]) for line in out.splitlines() if line.startswith("JSON ")), None)
        if j is None:
            return {"skipped": "soil_ref_lean printed no JSON line"}
        js.append(j)
    tot = [sum(j[k] for k in ("t_water", "t_grid", "t_wind", "t_freq")) for j in js]
    return {"ms_per_tick": round(1e3 * (tot[1] - tot[0]) / ticks, 3), "water_steps_top": js[1]["steps_water_top"] - js[0]["steps_water_top"],
            "binary": "oracle/_ref/soil_ref_lean (the reference's own headers, g++ -O2, one process, one pinned core)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--no-record", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of the record (default: profiles/)")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--no-standalone", action="store_true")
    a = ap.parse_args()
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    rec = {"workload": {"soil": SOIL, "size": SIZE, "nwater": NWATER, "nwind": NWIND, "seeds": "0..B-1", "pool_sections_per_cell": 8,
                        "warmup": a.warmup, "ticks": a.ticks}}
    if not a.no_standalone:
        rec["standalone_serial"] = run_standalone(cfg, a.warmup, a.ticks)
    rows = []
    for b in (int(x) for x in a.batches.split(",") if x):
        r = run_ensemble(cfg, b, a.warmup, a.ticks)
        rows.append(r)
        print(f"[ensemble] B={b:5d}  {r['ms_per_tick']:9.2f} ms/tick  {r['water_steps_per_s'] / 1e6:8.3f} M water steps/s", file=sys.stderr, flush=True)
    base = next((r for r in rows if r["members"] == 1), None)
    for r in rows:
        if base:
            r["slowdown_per_member_vs_b1"] = round(r["ms_per_tick"] / base["ms_per_tick"], 3)
            r["throughput_vs_b1"] = round(r["members"] * base["ms_per_tick"] / r["ms_per_tick"], 2)
    rec["ensembles"] = rows
    if not a.no_ref:
        ref = run_reference(a.warmup, a.ticks)
        rec["reference_one_core"] = ref
        if "ms_per_tick" in ref:
            for r in rows:
                r["host_cores_equivalent"] = round(r["members"] * ref["ms_per_tick"] / r["ms_per_tick"], 2)
    floors = {}
    sa = rec.get("standalone_serial")
    if base and sa:
        floors["b1_within_10pct_of_standalone"] = base["ms_per_tick"] <= 1.10 * sa["ms_per_tick"]
        floors["b1_over_standalone"] = round(base["ms_per_tick"] / sa["ms_per_tick"], 3)
    r256 = next((r for r in rows if r["members"] == 256), None)
    if base and r256:
        floors["b256_at_most_8x_b1"] = r256["ms_per_tick"] <= 8.0 * base["ms_per_tick"]
        floors["b256_over_b1"] = round(r256["ms_per_tick"] / base["ms_per_tick"], 3)
    rec["floors"] = floors
    line = json.dumps(rec)
    print(line, flush=True)
    if not a.no_record:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"r07_ensemble_{a.tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
