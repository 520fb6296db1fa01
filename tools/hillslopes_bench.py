#!/usr/bin/env python3
"""The hillslopes (smx_hillslopes) timed on the device. Prints one JSON line and writes <out>/r20_hillslopes_<tag>.json.

usage: hillslopes_bench.py [--size 4096] [--ticks 20] [--thresholds 16,256,4096] [--calls 10] [--warmup 3] [--trace-calls 0] [--tag bench] [--out profiles]
       hillslopes_bench.py --split <dir>

A `default.soil` map of size^2 spun up on the relaxed engine with bench.py's area-scaled particle counts for `ticks` ticks. In the
same run, on the same state, through ctypes into buffers made once (the C-ABI's own cost, no Python record):
  hillslopes_records      smx_hillslopes(threshold) with cap = the segment count known from a first call and no plane
  hillslopes_all_planes   the same with entry, hillslope, straight, diagonal and hand: five plane copies to the host
  streams_segments        smx_streams(threshold) with cap = the segment count and the segments plane: the yardstick -- the hillslope
                          call runs the same launches before its own
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host, and starts on an
idle stream); `warmup` calls of each first (the first one allocates the scratch), then `calls` rounds of the three in turns: the
median (min, max) of each.

Per-kernel times come from a run of their own under the profiler, which then holds nothing but the calls to be split up:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/hillslopes_bench.py --trace-calls 5
  python tools/hillslopes_bench.py --split <dir>
With --trace-calls N the timed section is replaced by one counting call and N records-only smx_hillslopes calls per threshold.
--split reads the per-dispatch trace: a call's rounds of k_hill_jump lie between its k_hill_init and its k_hill_fold, and their number
names the threshold (the smallest k with 2^k >= min(threshold, cells) - 1)."""
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
PLANES = ("entry", "hillslope", "straight", "diagonal", "hand")


def c_hillslopes(m, threshold: int, cap: int, planes: tuple):
    from soilmachine_amd import capi
    out = (capi.Hillslope * max(1, cap))()
    n = C.c_uint32()
    buf = {k: np.zeros(m.dimx * m.dimy, np.float64 if k == "hand" else np.uint32) for k in planes}
    args = [capi.ptr(buf.get(k)) for k in PLANES]
    return lambda: m._chk(m.L.smx_hillslopes(m.h, threshold, out, C.sizeof(capi.Hillslope), cap, C.byref(n), *args))


def c_streams_segments(m, threshold: int, cap: int):
    from soilmachine_amd import capi
    out = (capi.Stream * max(1, cap))()
    n = C.c_uint32()
    seg = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_streams(m.h, threshold, out, C.sizeof(capi.Stream), cap, C.byref(n), None, capi.ptr(seg), None, None))


def rounds_of(threshold: int, cells: int) -> int:
    k = 0
    while (1 << k) < min(threshold, cells) - 1:
        k += 1
    return k


def split(d: str) -> dict:
    """The per-dispatch kernel trace under `d` -> per number of rounds in a call: the calls, and the mean, min and max duration (ms) of
    k_hill_init, of one k_hill_jump round and of k_hill_fold."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + d)
    rows = []
    for r in csv.DictReader(open(f[0])):
        name = r["Kernel_Name"]
        kind = next((k for k in ("k_hill_init", "k_hill_jump", "k_hill_fold") if k in name), None)
        if kind:
            rows.append((int(r["Start_Timestamp"]), kind, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    calls, cur = {}, None
    for _, kind, ms in rows:
        if kind == "k_hill_init":
            cur = {"k_hill_init": [ms], "k_hill_jump": [], "k_hill_fold": []}
        elif cur is not None:
            cur[kind].append(ms)
            if kind == "k_hill_fold":
                g = calls.setdefault(len(cur["k_hill_jump"]), {"calls": 0, "k_hill_init": [], "k_hill_jump": [], "k_hill_fold": []})
                g["calls"] += 1
                for k in ("k_hill_init", "k_hill_jump", "k_hill_fold"):
                    g[k] += cur[k]
                cur = None
    out = {}
    for k, g in sorted(calls.items()):
        out[k] = {"calls": g["calls"]}
        for name in ("k_hill_init", "k_hill_jump", "k_hill_fold"):
            v = g[name]
            out[k][name] = {"n": len(v), "mean_ms": round(statistics.mean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} if v else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--thresholds", default="16,256,4096")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--split", default="")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.split:
        print(json.dumps({"rounds": split(a.split)}), flush=True)
        return
    from soilmachine_amd import capi
    from soilmachine_amd.machine import Layermap
    from soilmachine_amd.soilfile import loadsoil
    thresholds = [int(x) for x in a.thresholds.split(",") if x]
    n = a.size
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    scale = (n / 256.0) ** 2
    nwater, nwind = int(250 * scale), int(250 * scale * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    for _ in range(a.ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    rec = {"soil": SOIL, "engine": "relaxed", "size": n, "ticks": a.ticks, "nwater": nwater, "nwind": nwind, "calls": a.calls, "warmup_calls": a.warmup,
           "thresholds": []}
    if a.trace_calls:
        for t in thresholds:
            ns = C.c_uint32()
            m._chk(m.L.smx_hillslopes(m.h, t, None, C.sizeof(capi.Hillslope), 0, C.byref(ns), None, None, None, None, None))
            f = c_hillslopes(m, t, int(ns.value), ())
            for _ in range(a.trace_calls):
                f()
        m.close()
        print(json.dumps({"traced_calls": a.trace_calls, "thresholds": thresholds, "rounds": [rounds_of(t, n * n) for t in thresholds], "size": n}), flush=True)
        return
    for t in thresholds:
        recs, planes = m.hillslopes(t, hillslope=True, straight=True, diagonal=True)
        ns = len(recs)
        steps = planes["straight"].astype(np.int64) + planes["diagonal"]
        row = {"threshold": t, "rounds": rounds_of(t, n * n), "segments": ns, "hillslope_cells": int(sum(r["cells"] for r in recs)),
               "largest_hillslope": max((r["cells"] for r in recs), default=0), "longest_path": int(steps.max()),
               "unchannelled_cells": int(((planes["hillslope"] == capi.HILL_NONE) & (steps > 0)).sum()),
               "flagged_records": sum(1 for r in recs if r["flags"])}
        del recs, planes, steps
        # the three calls in turns, so that whatever else the machine does meets them alike
        fs = {"hillslopes_records": c_hillslopes(m, t, ns, ()), "hillslopes_all_planes": c_hillslopes(m, t, ns, PLANES), "streams_segments": c_streams_segments(m, t, ns)}
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
        row["records_minus_streams_ms"] = round(row["hillslopes_records"]["wall_ms"] - row["streams_segments"]["wall_ms"], 4)
        rec["thresholds"].append(row)
        print(f"[hillslopes] {n}^2 threshold {t:5d} {row['rounds']:2d} rounds {ns:9d} segments  records {row['hillslopes_records']['wall_ms']:9.3f} ms  all planes "
              f"{row['hillslopes_all_planes']['wall_ms']:9.3f} ms  streams(segments) {row['streams_segments']['wall_ms']:9.3f} ms (wall clock)", file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r20_hillslopes_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
