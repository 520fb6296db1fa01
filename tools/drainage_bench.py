#!/usr/bin/env python3
"""Drainage (smx_drainage / smx_ensemble_drainage) timed on the device. Prints one JSON line and writes profiles/r13_drainage_<tag>.json.

usage: drainage_bench.py [--sizes 1024,4096] [--ticks 25] [--calls 10] [--warmup 3] [--members 64] [--no-ensemble] [--tag bench] [--out profiles]

Per size, a `default.soil` map spun up on the relaxed engine with bench.py's area-scaled particle counts for `ticks` ticks. In the
same run, on the same state:
  records        smx_drainage with cap = the basin count known from a first call and no plane, through ctypes into buffers made once
  all_planes     the same with receivers, labels and area: two more launches and three plane copies to the host
                 (also: counting only, receivers and labels, the area alone)
  lakes_census   smx_lakes with cap = the lake count: the census drainage contains, the yardstick
  python_drainage_records   Layermap.drainage(cap): the same call plus one Python dict per record
  snapshot       Layermap.snapshot(): what a caller paid before any host loop could start
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host); `warmup` calls
first (the first one allocates the scratch), then the median (min, max) of `calls`. The ensemble line: `members` maps of 256^2 `default.soil` after 10
ticks, smx_ensemble_drainage in one call against smx_drainage member by member, the same cap."""
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
from soilmachine_amd.ensemble import Ensemble          # noqa: E402
from soilmachine_amd.machine import Layermap           # noqa: E402
from soilmachine_amd.soilfile import loadsoil          # noqa: E402

SOIL = "default.soil"


def timed(fn, calls: int, warmup: int) -> dict:
    """fn() `warmup` + `calls` times; the wall clock around each timed call, in ms. Every call timed here blocks until its results
    are on the host (one synchronisation at its end) and starts on an idle stream, so the clock spans the device work."""
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
    return {"wall_ms": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}


def c_drainage(m: Layermap, cap: int, planes: tuple):
    """One smx_drainage call into buffers made once: the C-ABI's own cost, without the Python records."""
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    buf = {k: np.zeros(m.dimx * m.dimy, np.uint32) for k in planes}
    args = [capi.ptr(buf.get(k)) for k in ("receivers", "labels", "area")]
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), *args))


def c_lakes(m: Layermap, cap: int):
    out = (capi.Lake * max(1, cap))()
    n = C.c_uint32()
    return lambda: m._chk(m.L.smx_lakes(m.h, out, C.sizeof(capi.Lake), cap, C.byref(n), None))


def run_size(n: int, ticks: int, calls: int, warmup: int) -> dict:
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    area = (n / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    recs, planes = m.drainage(area=True)
    lakes = m.lakes()
    nb, nl = len(recs), len(lakes)
    sinks = [r for r in recs if not r["flags"] & capi.BASIN_LAKE]
    out = {"size": n, "nwater": nwater, "nwind": nwind, "ticks": ticks, "basins": nb, "lakes": nl, "sinks": len(sinks),
           "sinks_on_the_border": sum(1 for r in sinks if r["flags"] & capi.BASIN_BORDER),
           "cells_in_lake_basins": int(sum(r["cells"] for r in recs if r["flags"] & capi.BASIN_LAKE)), "largest_area": int(planes["area"].max()),
           "records": timed(c_drainage(m, nb, ()), calls, warmup),
           "count_only": timed(c_drainage(m, 0, ()), calls, warmup),
           "receivers_and_labels": timed(c_drainage(m, nb, ("receivers", "labels")), calls, warmup),
           "all_planes": timed(c_drainage(m, nb, ("receivers", "labels", "area")), calls, warmup),
           "area_only": timed(c_drainage(m, nb, ("area",)), calls, warmup),
           "lakes_census": timed(c_lakes(m, nl), calls, warmup),
           "python_drainage_records": timed(lambda: m.drainage(cap=nb), calls, 1),
           "snapshot": timed(m.snapshot, max(2, calls // 3), 1)}
    m.close()
    return out


def run_ensemble(members: int, calls: int, warmup: int) -> dict:
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, 256, 256, seed=s, pool=8 * 256 * 256) for s in range(members)]
        ens.tick(250, 250, n=10)
        ens.sync()
        one = ens.drainage()
        each = [m.drainage() for m in mem]
        if one != each:
            raise SystemExit("Ensemble.drainage() and the member-by-member calls DISAGREE")
        cap = max(len(x) for x in one)
        out = (capi.Basin * (members * cap))()
        counts = np.zeros(members, np.uint32)
        singles = [c_drainage(m, cap, ()) for m in mem]

        def all_singles():
            for f in singles:
                f()

        row = {"members": members, "size": 256, "soil": SOIL, "ticks": 10, "basins_total": sum(len(x) for x in one), "cap": cap,
               "ensemble_call": timed(lambda: ens._chk(ens.L.smx_ensemble_drainage(ens.h, out, C.sizeof(capi.Basin), cap, capi.ptr(counts))), calls, warmup),
               "member_by_member": timed(all_singles, calls, warmup)}
        row["speedup_wall"] = round(row["member_by_member"]["wall_ms"] / row["ensemble_call"]["wall_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--ticks", type=int, default=25)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    rec = {"soil": SOIL, "engine": "relaxed", "calls": a.calls, "warmup_calls": a.warmup, "maps": []}
    for n in sizes:
        r = run_size(n, a.ticks, a.calls, a.warmup)
        rec["maps"].append(r)
        print(f"[drainage] {n}^2 {r['basins']:8d} basins  records {r['records']['wall_ms']:9.3f} ms  all planes {r['all_planes']['wall_ms']:9.3f} ms  "
              f"lakes {r['lakes_census']['wall_ms']:9.3f} ms  snapshot {r['snapshot']['wall_ms']:9.3f} ms (wall clock)", file=sys.stderr, flush=True)
    if not a.no_ensemble:
        rec["ensemble"] = e = run_ensemble(a.members, a.calls, a.warmup)
        print(f"[drainage] {e['members']} x 256^2: one call {e['ensemble_call']['wall_ms']:.3f} ms, member by member {e['member_by_member']['wall_ms']:.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r13_drainage_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
