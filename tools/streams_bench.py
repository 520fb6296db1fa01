#!/usr/bin/env python3
"""The stream network (smx_streams) timed on the device. Prints one JSON line and writes <out>/r16_streams_<tag>.json.

usage: streams_bench.py [--size 4096] [--ticks 20] [--thresholds 1,16,256] [--calls 10] [--warmup 3] [--trace-calls 0] [--tag bench] [--out profiles]

A `default.soil` map of size^2 spun up on the relaxed engine with bench.py's area-scaled particle counts for `ticks` ticks. In the
same run, on the same state, through ctypes into buffers made once (the C-ABI's own cost, no Python record):
  streams_records      smx_streams(threshold) with cap = the segment count known from a first call and no plane
  streams_all_planes   the same with order, segments, reach and heads: four plane copies to the host
  drainage_area        smx_drainage with cap = the basin count and the area plane alone: the yardstick -- the stream call runs the
                       same drainage launches (but for the basins' scan and statistics) before its own
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host); `warmup` calls
first (the first one allocates the scratch), then the median (min, max) of `calls`. ratio = streams / drainage_area, medians.

Per-kernel times come from a run of their own under the profiler, which then holds nothing but the calls to be split up:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/streams_bench.py --trace-calls 5 --thresholds 16
  python tools/kernel_stats.py <dir>
With --trace-calls N the timed section is replaced by N records-only smx_streams calls per threshold and N drainage_area calls."""
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
PLANES = ("order", "segments", "reach", "heads")


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


def c_streams(m: Layermap, threshold: int, cap: int, planes: tuple):
    out = (capi.Stream * max(1, cap))()
    n = C.c_uint32()
    buf = {k: np.zeros(m.dimx * m.dimy, np.uint32) for k in planes}
    args = [capi.ptr(buf.get(k)) for k in PLANES]
    return lambda: m._chk(m.L.smx_streams(m.h, threshold, out, C.sizeof(capi.Stream), cap, C.byref(n), *args))


def c_drainage_area(m: Layermap, cap: int):
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    area = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, None, capi.ptr(area)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--thresholds", default="1,16,256")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    thresholds = [int(x) for x in a.thresholds.split(",") if x]
    n = a.size
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    scale = (n / 256.0) ** 2
    nwater, nwind = int(250 * scale), int(250 * scale * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    for _ in range(a.ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    nb = C.c_uint32()
    m._chk(m.L.smx_drainage(m.h, None, C.sizeof(capi.Basin), 0, C.byref(nb), None, None, None))
    rec = {"soil": SOIL, "engine": "relaxed", "size": n, "ticks": a.ticks, "nwater": nwater, "nwind": nwind, "calls": a.calls, "warmup_calls": a.warmup,
           "basins": int(nb.value), "thresholds": []}
    if a.trace_calls:
        for t in thresholds:
            ns = C.c_uint32()
            m._chk(m.L.smx_streams(m.h, t, None, C.sizeof(capi.Stream), 0, C.byref(ns), None, None, None, None))
            f = c_streams(m, t, int(ns.value), ())
            for _ in range(a.trace_calls):
                f()
        f = c_drainage_area(m, int(nb.value))
        for _ in range(a.trace_calls):
            f()
        m.close()
        print(json.dumps({"traced_calls": a.trace_calls, "thresholds": thresholds, "size": n}), flush=True)
        return
    rec["drainage_area"] = d = timed(c_drainage_area(m, int(nb.value)), a.calls, a.warmup)
    for t in thresholds:
        recs, planes = m.streams(t, order=True, reach=True)
        ns = len(recs)
        row = {"threshold": t, "segments": ns, "largest_order": max((r["order"] for r in recs), default=0), "largest_reach": int(planes["reach"].max()),
               "longest_segment": max((r["cells"] for r in recs), default=0), "channel_cells": int((planes["order"] != 0).sum()),
               "streams_records": timed(c_streams(m, t, ns, ()), a.calls, a.warmup),
               "streams_all_planes": timed(c_streams(m, t, ns, PLANES), a.calls, a.warmup)}
        del recs, planes
        row["ratio_records"] = round(row["streams_records"]["wall_ms"] / d["wall_ms"], 3)
        row["ratio_all_planes"] = round(row["streams_all_planes"]["wall_ms"] / d["wall_ms"], 3)
        rec["thresholds"].append(row)
        print(f"[streams] {n}^2 threshold {t:4d} {ns:9d} segments  records {row['streams_records']['wall_ms']:9.3f} ms  all planes "
              f"{row['streams_all_planes']['wall_ms']:9.3f} ms  drainage(area) {d['wall_ms']:9.3f} ms (wall clock)", file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r16_streams_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
