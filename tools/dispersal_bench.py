#!/usr/bin/env python3
"""Dispersed flow (smx_dispersal) timed on the device. Prints one JSON line and writes <out>/r22_dispersal_<tag>.json.

usage: dispersal_bench.py [--size 4096] [--ticks 0,20] [--calls 5] [--warmup 2] [--trace-calls 0] [--tag bench] [--out profiles]
       dispersal_bench.py --split <dir>

A `default.soil` map of size^2, on the initial terrain (ticks 0) and spun up on the relaxed engine with bench.py's area-scaled
particle counts (ticks 20). In the same run, on the same state, through ctypes into buffers made once (the C-ABI's own cost, no
Python record):
  dispersal_e1_records   smx_dispersal(exponent 1) with cap = the basin count known from a first call, no plane
  dispersal_e1_planes    the same with the three planes: three plane copies to the host
  dispersal_e4_records / dispersal_e4_planes   the same with exponent 4
  drainage_area          smx_drainage with cap = the basin count and the area plane: the chain and the D8 walk, the yardstick
Times: the wall clock around the blocking call (it ends in its last synchronisation, with the results on the host, and starts on an
idle stream); `warmup` calls of each first (the first one allocates the scratch), then `calls` rounds of the five in turns: the
median (min, max) of each. With them the rounds and batches of the call (smx_get_dispersal_rounds) and the largest `peak` against
drainage's largest area.

Per-kernel times come from a run of their own under the profiler, which then holds nothing but the calls to be split up:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/dispersal_bench.py --trace-calls 3
  python tools/dispersal_bench.py --split <dir>
With --trace-calls N the timed section is replaced by one counting call and N records-only smx_dispersal(exponent 1) calls per
state, followed by N smx_drainage calls with the area plane. --split reads the per-dispatch trace: the dispatches and the total,
mean, min and max duration of every k_disp_* kernel and of the chain's kernels."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOIL = "default.soil"
PLANES = ("area", "donors", "receivers")
KERNELS = ("k_disp_pending", "k_disp_flow", "k_disp_fold", "k_disp_peak", "k_drain_pending", "k_drain_area", "k_drain_stats", "k_drain_resolve", "k_drain_recv",
           "k_lake_tiles", "k_lake_merge", "k_lake_flatten")


def c_dispersal(m, exponent: int, cap: int, planes: tuple):
    from soilmachine_amd import capi
    out = (capi.Dispersal * max(1, cap))()
    n = C.c_uint32()
    cells = m.dimx * m.dimy
    buf = {k: np.zeros(cells, np.uint64 if k == "area" else np.uint32) for k in planes}
    args = [capi.ptr(buf.get(k)) for k in PLANES]
    return lambda: m._chk(m.L.smx_dispersal(m.h, exponent, out, C.sizeof(capi.Dispersal), cap, C.byref(n), *args))


def c_drainage_area(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    area = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, None, capi.ptr(area)))


def split(d: str) -> dict:
    """The per-dispatch kernel trace under `d` -> per kernel of KERNELS: the dispatches and the total, mean, min and max duration (ms)."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + d)
    got = {k: [] for k in KERNELS}
    for r in csv.DictReader(open(f[0])):
        kind = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if kind:
            got[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return {k: {"n": len(v), "total_ms": round(sum(v), 3), "mean_ms": round(statistics.mean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in got.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ticks", default="0,20")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--split", default="")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.split:
        print(json.dumps({"kernels": split(a.split)}), flush=True)
        return
    from soilmachine_amd import capi
    from soilmachine_amd.machine import Layermap
    from soilmachine_amd.soilfile import loadsoil
    states = [int(x) for x in a.ticks.split(",") if x]
    n = a.size
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    scale = (n / 256.0) ** 2
    nwater, nwind = int(250 * scale), int(250 * scale * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    rec = {"soil": SOIL, "engine": "relaxed", "size": n, "nwater": nwater, "nwind": nwind, "calls": a.calls, "warmup_calls": a.warmup, "states": []}
    done = 0
    for ticks in sorted(states):
        for _ in range(ticks - done):
            m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
        done = ticks
        m.sync()
        nb = C.c_uint32()
        m._chk(m.L.smx_drainage(m.h, None, C.sizeof(capi.Basin), 0, C.byref(nb), None, None, None))
        nb = int(nb.value)
        if a.trace_calls:
            for f in (c_dispersal(m, 1, nb, ()), c_drainage_area(m, nb)):
                for _ in range(a.trace_calls):
                    f()
            rec["states"].append({"ticks": ticks, "basins": nb, "traced_calls": a.trace_calls})
            continue
        row = {"ticks": ticks, "basins": nb}
        t0 = time.perf_counter()
        m._chk(m.L.smx_dispersal(m.h, 1, None, C.sizeof(capi.Dispersal), 0, C.byref(C.c_uint32()), None, None, None))   # (allocates the scratch)
        row["first_call_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        print(f"[dispersal] {n}^2 after {ticks} ticks: the first call {row['first_call_ms']} ms, rounds and batches {m.dispersal_rounds()}", file=sys.stderr, flush=True)
        drecs, dp = m.drainage(area=True)
        for e in (1, 4):
            recs = m.dispersal(e)
            rounds, batches = m.dispersal_rounds()
            row[f"e{e}"] = {"rounds": rounds, "batches": batches, "largest_peak_cells": max(r["peak"] for r in recs), "largest_leak_out_cells": max(r["leak_out"] for r in recs),
                            "givers": sum(r["givers"] for r in recs), "split_cells": sum(r["split_cells"] for r in recs),
                            "inflows_sum_to_the_map": sum(r["inflow_q24"] for r in recs) == n * n << 24}
            del recs
        row["drainage_largest_area"] = int(dp["area"].max())
        row["lake_basins"] = sum(1 for r in drecs if r["flags"] & capi.BASIN_LAKE)
        del drecs, dp
        # the calls in turns, so that whatever else the machine does meets them alike
        fs = {"dispersal_e1_records": c_dispersal(m, 1, nb, ()), "dispersal_e1_planes": c_dispersal(m, 1, nb, PLANES),
              "dispersal_e4_records": c_dispersal(m, 4, nb, ()), "dispersal_e4_planes": c_dispersal(m, 4, nb, PLANES), "drainage_area": c_drainage_area(m, nb)}
        for f in fs.values():
            for _ in range(a.warmup):
                f()
        wall = {k: [] for k in fs}
        for _ in range(a.calls):
            for k, f in fs.items():
                t0 = time.perf_counter()
                f()
                wall[k].append(1e3 * (time.perf_counter() - t0))
        for k, w in wall.items():
            row[k] = {"wall_ms": round(statistics.median(w), 4), "wall_ms_min": round(min(w), 4), "wall_ms_max": round(max(w), 4)}
        rec["states"].append(row)
        print(f"[dispersal] {n}^2 after {ticks:3d} ticks {nb:9d} basins  " + "  ".join(f"{k} {row[k]['wall_ms']:9.3f} ms" for k in fs) + " (wall clock)",
              file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    if not a.trace_calls:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"r22_dispersal_{a.tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
