#!/usr/bin/env python3
"""Through-drainage (smx_through) timed on the device. Prints one JSON line and writes profiles/r18_through_<tag>.json.

usage: through_bench.py [--sizes 1024,4096] [--ticks 20] [--calls 10] [--warmup 3] [--tag bench] [--out profiles]

Per size, a `default.soil` map on the relaxed engine, measured twice in the same run: on the INITIAL terrain, and after `ticks` ticks
with bench.py's area-scaled particle counts. On each state:
  records        smx_through with cap = the basin count and no plane, through ctypes into buffers made once
  with_planes    the same with through_area and outlets: k_drain_pending, k_through_plane, k_through_area and the two copies more
  level_sweeps, hop_sweeps, batches   smx_get_through_sweeps after the call
  max_hops, roots, largest_through_cells, largest_through_area, largest_area   what the records and the planes hold
  spill_records  smx_spill (records) on the same state: the chain smx_through contains, sweeps of the levels included
  drainage_area  smx_drainage with the area plane on the same state: the other yardstick, the walk smx_through ends with
Times: the wall clock around the blocking call; `warmup` calls first (the first one allocates the scratch), then the median (min,
max) of `calls`."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soilmachine_amd import capi                       # noqa: E402
from soilmachine_amd.machine import Layermap           # noqa: E402
from soilmachine_amd.soilfile import loadsoil          # noqa: E402

SOIL = "default.soil"


def timed(fn, calls: int, warmup: int) -> dict:
    """fn() `warmup` + `calls` times; the wall clock around each timed call, in ms. Every call timed here blocks until its results
    are on the host and starts on an idle stream, so the clock spans the device work."""
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
    return {"wall_ms": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}


def c_through(m: Layermap, cap: int, planes: bool):
    """One smx_through call into buffers made once: the C-ABI's own cost, without the Python records."""
    out = (capi.Through * max(1, cap))()
    n = C.c_uint32()
    area = np.zeros(m.dimx * m.dimy, np.uint32) if planes else None
    outlets = np.zeros(m.dimx * m.dimy, np.uint32) if planes else None
    return lambda: m._chk(m.L.smx_through(m.h, out, C.sizeof(capi.Through), cap, C.byref(n), capi.ptr(area), capi.ptr(outlets)))


def c_spill(m: Layermap, cap: int):
    out = (capi.Spill * max(1, cap))()
    n = C.c_uint32()
    return lambda: m._chk(m.L.smx_spill(m.h, out, C.sizeof(capi.Spill), cap, C.byref(n), None))


def c_drainage_area(m: Layermap, cap: int):
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    area = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, None, capi.ptr(area)))


def measure(m: Layermap, state: str, calls: int, warmup: int) -> dict:
    recs, planes = m.through(area=True, outlets=True)
    nb = len(recs)
    _, dplanes = m.drainage(area=True)
    row = {"state": state, "basins": nb, "lake_basins": sum(1 for r in recs if r["flags"] & capi.THROUGH_LAKE),
           "roots": sum(1 for r in recs if r["flags"] & capi.THROUGH_OFFMAP), "not_the_pour_point": sum(1 for r in recs if r["flags"] & capi.THROUGH_NOT_POUR),
           "wet_entries": sum(1 for r in recs if r["flags"] & capi.THROUGH_WET_ENTRY), "max_hops": max(r["hops"] for r in recs),
           "largest_through_cells": max(r["through_cells"] for r in recs), "largest_cells": max(r["cells"] for r in recs),
           "largest_through_area": int(planes["through_area"].max()), "largest_area": int(dplanes["area"].max()),
           "roots_sum": sum(r["through_cells"] for r in recs if r["flags"] & capi.THROUGH_OFFMAP)}
    del recs, planes, dplanes
    row["records"] = timed(c_through(m, nb, False), calls, warmup)
    row["level_sweeps"], row["hop_sweeps"], row["batches"] = m.through_sweeps()
    row["with_planes"] = timed(c_through(m, nb, True), calls, warmup)
    row["spill_records"] = timed(c_spill(m, nb), calls, warmup)
    row["spill_sweeps"] = m.spill_sweeps()[0]
    row["drainage_area"] = timed(c_drainage_area(m, nb), calls, warmup)
    return row


def run_size(n: int, ticks: int, calls: int, warmup: int) -> dict:
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    area = (n / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    out = {"size": n, "nwater": nwater, "nwind": nwind, "ticks": ticks, "states": [measure(m, "initial terrain", calls, warmup)]}
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    out["states"].append(measure(m, f"after {ticks} relaxed ticks", calls, warmup))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    rec = {"soil": SOIL, "engine": "relaxed", "calls": a.calls, "warmup_calls": a.warmup, "maps": []}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        r = run_size(n, a.ticks, a.calls, a.warmup)
        rec["maps"].append(r)
        for s in r["states"]:
            print(f"[through] {n}^2 {s['state']:24s} {s['basins']:8d} basins {s['roots']:7d} roots  max hops {s['max_hops']:5d}  records {s['records']['wall_ms']:9.3f} ms  "
                  f"with planes {s['with_planes']['wall_ms']:9.3f} ms  {s['level_sweeps']} level + {s['hop_sweeps']} hop sweeps in {s['batches']} batches  "
                  f"spill {s['spill_records']['wall_ms']:9.3f} ms  drainage+area {s['drainage_area']['wall_ms']:9.3f} ms (wall clock)", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r18_through_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
