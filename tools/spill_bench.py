#!/usr/bin/env python3
"""Spill analysis (smx_spill) timed on the device. Prints one JSON line and writes profiles/r17_spill_<tag>.json.

usage: spill_bench.py [--sizes 4096] [--ticks 20] [--calls 10] [--warmup 3] [--no-snapshot] [--tag bench] [--out profiles]

Per size, a `default.soil` map on the relaxed engine, measured twice in the same run: on the INITIAL terrain, and after `ticks` ticks
with bench.py's area-scaled particle counts. On each state:
  records        smx_spill with cap = the basin count and no plane, through ctypes into buffers made once
  with_filled    the same with the filled plane: one more pass over the plane in k_spill_store and its copy to the host
  count_only     cap 0, out NULL: the whole chain runs (the fill levels are not cut short), only the copy of the records is saved
  sweeps, batches   smx_get_spill_sweeps after the call: relax sweeps launched, host looks at the change counts
  drainage_labels   smx_drainage with the label plane on the same state: the yardstick, the chain smx_spill starts with
  snapshot       Layermap.snapshot(): what a caller paid before a priority flood on the host could start
Times: the wall clock around the blocking call; `warmup` calls first (the first one allocates the scratch), then the median (min,
max) of `calls`. The kernels' shares come from a run of this tool under a kernel trace (tools/kernel_stats.py)."""
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


def c_spill(m: Layermap, cap: int, filled: bool):
    """One smx_spill call into buffers made once: the C-ABI's own cost, without the Python records."""
    out = (capi.Spill * max(1, cap))()
    n = C.c_uint32()
    plane = np.zeros(m.dimx * m.dimy, np.float64) if filled else None
    return lambda: m._chk(m.L.smx_spill(m.h, out if cap else None, C.sizeof(capi.Spill), cap, C.byref(n), capi.ptr(plane)))


def c_drainage_labels(m: Layermap, cap: int):
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    labels = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, capi.ptr(labels), None))


def measure(m: Layermap, state: str, calls: int, warmup: int, snapshot: bool) -> dict:
    recs = m.spill()
    nb = len(recs)
    row = {"state": state, "basins": nb, "lake_basins": sum(1 for r in recs if r["flags"] & capi.SPILL_LAKE),
           "pour_off_the_map": sum(1 for r in recs if r["flags"] & capi.SPILL_OFFMAP), "nested": sum(1 for r in recs if r["flags"] & capi.SPILL_NESTED),
           "unreliable": sum(1 for r in recs if r["flags"] & (capi.SPILL_STORAGE_UNRELIABLE | capi.SPILL_FILL_STORAGE_UNRELIABLE)),
           "storage": sum(r["storage"] for r in recs), "fill_storage": sum(r["fill_storage"] for r in recs),
           "records": timed(c_spill(m, nb, False), calls, warmup)}
    row["sweeps"], row["batches"] = m.spill_sweeps()
    row["with_filled"] = timed(c_spill(m, nb, True), calls, warmup)
    row["count_only"] = timed(c_spill(m, 0, False), calls, warmup)
    row["drainage_labels"] = timed(c_drainage_labels(m, nb), calls, warmup)
    if snapshot:
        row["snapshot"] = timed(m.snapshot, max(2, calls // 3), 1)
    del recs
    return row


def run_size(n: int, ticks: int, calls: int, warmup: int, snapshot: bool) -> dict:
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    area = (n / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    out = {"size": n, "nwater": nwater, "nwind": nwind, "ticks": ticks, "states": [measure(m, "initial terrain", calls, warmup, snapshot)]}
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    out["states"].append(measure(m, f"after {ticks} relaxed ticks", calls, warmup, snapshot))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-snapshot", action="store_true")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    rec = {"soil": SOIL, "engine": "relaxed", "calls": a.calls, "warmup_calls": a.warmup, "maps": []}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        r = run_size(n, a.ticks, a.calls, a.warmup, not a.no_snapshot)
        rec["maps"].append(r)
        for s in r["states"]:
            print(f"[spill] {n}^2 {s['state']:24s} {s['basins']:8d} basins  records {s['records']['wall_ms']:9.3f} ms  with filled {s['with_filled']['wall_ms']:9.3f} ms  "
                  f"{s['sweeps']} sweeps in {s['batches']} batches  drainage+labels {s['drainage_labels']['wall_ms']:9.3f} ms (wall clock)", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r17_spill_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
