#!/usr/bin/env python3
"""The flow paths (smx_flowpaths) timed on the device. Prints one JSON line and writes <out>/r21_flowpaths_<tag>.json.

usage: flowpaths_bench.py [--size 4096] [--ticks 0,20] [--calls 10] [--warmup 3] [--trace-calls 0] [--tag bench] [--out profiles]
       flowpaths_bench.py --split <dir>

A `default.soil` map of size^2, on the initial terrain (ticks 0) and spun up on the relaxed engine with bench.py's area-scaled
particle counts (ticks 20). In the same run, on the same state, through ctypes into buffers made once (the C-ABI's own cost, no
Python record):
  flowpaths_records      smx_flowpaths with cap = the basin count known from a first call, no plane, no profile
  flowpaths_all_planes   the same with the seven planes: seven plane copies to the host
  flowpaths_profile      records and the profile, no plane
  drainage_area          smx_drainage with cap = the basin count and the area plane: the chain and the leaf-to-terminal walk
  hillslopes_no_channel  smx_hillslopes(threshold = cells + 1), records only: the same number of jump rounds
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host, and starts on an
idle stream); `warmup` calls of each first (the first one allocates the scratch), then `calls` rounds of the five in turns: the
median (min, max) of each.

Per-kernel times come from a run of their own under the profiler, which then holds nothing but the calls to be split up:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/flowpaths_bench.py --trace-calls 5
  python tools/flowpaths_bench.py --split <dir>
With --trace-calls N the timed section is replaced by one counting call and N records-only smx_flowpaths calls per state, followed
by N smx_drainage calls with the area plane. --split reads the per-dispatch trace: the mean, min and max duration of every k_path_*
kernel, of one k_hill_jump round, and of k_drain_pending and k_drain_area."""
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
PLANES = ("terminal", "straight", "diagonal", "drop", "upstream", "source", "stem")
KERNELS = ("k_path_init", "k_hill_jump", "k_path_fold", "k_path_up", "k_path_lengths", "k_path_stem", "k_drain_pending", "k_drain_area", "k_drain_stats",
           "k_drain_resolve", "k_drain_recv")


def c_flowpaths(m, cap: int, planes: tuple, profile: bool):
    from soilmachine_amd import capi
    out = (capi.Flowpath * max(1, cap))()
    n, npr = C.c_uint32(), C.c_uint32()
    cells = m.dimx * m.dimy
    buf = {k: np.zeros(cells, np.float64 if k == "drop" else np.uint32) for k in planes}
    prof = np.zeros(cells if profile else 1, np.uint32)
    args = [capi.ptr(buf.get(k)) for k in PLANES] + [capi.ptr(prof) if profile else None, cells if profile else 0, C.byref(npr)]
    return lambda: m._chk(m.L.smx_flowpaths(m.h, out, C.sizeof(capi.Flowpath), cap, C.byref(n), *args))


def c_drainage_area(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    area = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, None, capi.ptr(area)))


def c_hillslopes_no_channel(m):
    from soilmachine_amd import capi
    out = (capi.Hillslope * 1)()
    n = C.c_uint32()
    t = m.dimx * m.dimy + 1
    return lambda: m._chk(m.L.smx_hillslopes(m.h, t, out, C.sizeof(capi.Hillslope), 1, C.byref(n), None, None, None, None, None))


def rounds_of(cells: int) -> int:
    k = 0
    while (1 << k) < cells - 1:
        k += 1
    return k


def split(d: str) -> dict:
    """The per-dispatch kernel trace under `d` -> per kernel of KERNELS: the dispatches and the mean, min and max duration (ms)."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + d)
    got = {k: [] for k in KERNELS}
    for r in csv.DictReader(open(f[0])):
        kind = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if kind:
            got[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return {k: {"n": len(v), "mean_ms": round(statistics.mean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in got.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ticks", default="0,20")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
    rec = {"soil": SOIL, "engine": "relaxed", "size": n, "rounds": rounds_of(n * n), "nwater": nwater, "nwind": nwind, "calls": a.calls, "warmup_calls": a.warmup,
           "states": []}
    done = 0
    for ticks in sorted(states):
        for _ in range(ticks - done):
            m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
        done = ticks
        m.sync()
        nb, npr = C.c_uint32(), C.c_uint32()
        m._chk(m.L.smx_flowpaths(m.h, None, C.sizeof(capi.Flowpath), 0, C.byref(nb), *[None] * 7, None, 0, C.byref(npr)))
        nb, npr = int(nb.value), int(npr.value)
        if a.trace_calls:
            for f in (c_flowpaths(m, nb, (), False), c_drainage_area(m, nb)):
                for _ in range(a.trace_calls):
                    f()
            rec["states"].append({"ticks": ticks, "basins": nb, "profile_cells": npr, "traced_calls": a.trace_calls})
            continue
        recs = m.flowpaths()
        row = {"ticks": ticks, "basins": nb, "profile_cells": npr, "longest_stem_steps": max(r["steps_max"] for r in recs),
               "largest_basin": max(r["cells"] for r in recs), "lake_basins": sum(1 for r in recs if r["flags"] & capi.PATH_TERMINAL_WET)}
        del recs
        # the calls in turns, so that whatever else the machine does meets them alike
        fs = {"flowpaths_records": c_flowpaths(m, nb, (), False), "flowpaths_all_planes": c_flowpaths(m, nb, PLANES, False),
              "flowpaths_profile": c_flowpaths(m, nb, (), True), "drainage_area": c_drainage_area(m, nb), "hillslopes_no_channel": c_hillslopes_no_channel(m)}
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
        print(f"[flowpaths] {n}^2 after {ticks:3d} ticks {nb:9d} basins  " + "  ".join(f"{k} {row[k]['wall_ms']:9.3f} ms" for k in fs) + " (wall clock)",
              file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    if not a.trace_calls:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"r21_flowpaths_{a.tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
