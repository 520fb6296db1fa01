#!/usr/bin/env python3
"""The catchments of listed outlets (smx_catchments) timed on the device. Prints one JSON line and writes <out>/r24_catchments_<tag>.json
and <out>/r24_catchments_<tag>.md, the tables of profiles/r24_catchments.md.

usage: catchments_bench.py [--size 4096] [--ticks 0,20] [--calls 10] [--warmup 3] [--trace-calls 0] [--tag bench] [--out profiles]
       catchments_bench.py --split <dir>

A `rockgravelpebblessand.soil` map of size^2, on the initial terrain (ticks 0) and spun up on the relaxed engine with bench.py's
area-scaled particle counts (ticks 20). In the same run, on the same state, through ctypes into buffers made once (the C-ABI's own
cost, no Python record), for each of four gauge lists -- 16, 4096 and 65 536 seeded random cells and the last cells of all
streams(256) segments:
  records      smx_catchments, no bins, no plane
  bins32       the same with 32 bins (bin_height: the largest finite drop of the list's own catchments / 32)
  all_planes   records and the four planes: four plane copies to the host
and beside them, once per state:
  drainage_labels     smx_drainage with cap = the basin count and the label plane: the yardstick, the chain the catchments start with
  flowpaths_records   smx_flowpaths, records only, for orientation: the same number of jump rounds
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host, and starts on an
idle stream); `warmup` calls of each first (the first one allocates the scratch), then `calls` rounds of all of them in turns: the
median (min, max) of each.

Per-kernel times come from a run of their own under the profiler, which then holds nothing but the calls to be split up:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/catchments_bench.py --trace-calls 5
  python tools/catchments_bench.py --split <dir>
With --trace-calls N the timed section is replaced by N records-only and N bins32 calls per list and state, followed by N
smx_drainage calls with the label plane. --split reads the per-dispatch trace: the mean, min and max duration of every k_catch_*
kernel, of one k_hill_jump round and of the chain's kernels."""
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

SOIL = "rockgravelpebblessand.soil"
PLANES = ("gauge", "straight", "diagonal", "drop")
KERNELS = ("k_catch_mark", "k_catch_init", "k_hill_jump", "k_catch_fold", "k_catch_hist", "k_drain_stats", "k_drain_resolve", "k_drain_recv", "k_lake_tiles", "k_lake_merge",
           "k_lake_flatten")
BINS = 32


def c_catchments(m, cells: np.ndarray, bins: int, bin_height: float, planes: tuple):
    from soilmachine_amd import capi
    n = len(cells)
    out = (capi.Catchment * n)()
    hist = np.zeros(max(1, n * bins), np.uint32)
    buf = {k: np.zeros(m.dimx * m.dimy, np.float64 if k == "drop" else np.uint32) for k in planes}
    args = [capi.ptr(buf.get(k)) for k in PLANES]
    return lambda: m._chk(m.L.smx_catchments(m.h, capi.ptr(cells), n, out, C.sizeof(capi.Catchment), capi.ptr(hist) if bins else None, bins, bin_height, *args))


def c_drainage_labels(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    labels = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, capi.ptr(labels), None))


def c_flowpaths_records(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Flowpath * max(1, cap))()
    n, npr = C.c_uint32(), C.c_uint32()
    return lambda: m._chk(m.L.smx_flowpaths(m.h, out, C.sizeof(capi.Flowpath), cap, C.byref(n), *[None] * 7, None, 0, C.byref(npr)))


def rounds_of(cells: int) -> int:
    k = 0
    while (1 << k) < cells - 1:
        k += 1
    return k


def gauge_lists(m, size: int) -> dict:
    """The four lists of a state: name -> distinct cells (uint32)."""
    rng = np.random.default_rng(24)
    cells = size * size
    lists = {f"random_{k}": np.ascontiguousarray(rng.choice(cells, min(k, cells), replace=False), np.uint32) for k in (16, 4096, 65536)}
    lists["stream_outlets_256"] = np.array([g["last_cell"] for g in m.streams(256)], np.uint32)
    return lists


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


def markdown(rec: dict) -> str:
    """The timing tables of a run."""
    out = [f"## {rec['size']}^2 `{rec['soil']}`, relaxed engine, {rec['rounds']} jump rounds, median (min .. max) of {rec['calls']} calls, wall clock in ms", ""]
    for st in rec["states"]:
        y = st["drainage_labels"]["wall_ms"]
        out += [f"### after {st['ticks']} ticks: {st['basins']} basins", "",
                f"`smx_drainage` with the label plane: {y:.3f} ({st['drainage_labels']['wall_ms_min']:.3f} .. {st['drainage_labels']['wall_ms_max']:.3f}); "
                f"`smx_flowpaths` records only: {st['flowpaths_records']['wall_ms']:.3f}", "",
                "| list | gauges | gauged cells | largest own | records | minus drainage | bins32 | all planes |", "|---|---|---|---|---|---|---|---|"]
        for name, row in st["lists"].items():
            f = lambda k: f"{row[k]['wall_ms']:.3f} ({row[k]['wall_ms_min']:.3f} .. {row[k]['wall_ms_max']:.3f})"
            out.append(f"| {name} | {row['gauges']} | {row['gauged_cells']} | {row['largest_own']} | {f('records')} | {row['records']['wall_ms'] - y:+.3f} | {f('bins32')} | "
                       f"{f('all_planes')} |")
        out.append("")
    return "\n".join(out)


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
           "bins": BINS, "states": []}
    done = 0
    for ticks in sorted(states):
        for _ in range(ticks - done):
            m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
        done = ticks
        m.sync()
        nb = C.c_uint32()
        m._chk(m.L.smx_drainage(m.h, None, C.sizeof(capi.Basin), 0, C.byref(nb), None, None, None))
        nb = int(nb.value)
        lists = gauge_lists(m, n)
        row = {"ticks": ticks, "basins": nb, "lists": {}}
        fs = {"drainage_labels": c_drainage_labels(m, nb), "flowpaths_records": c_flowpaths_records(m, nb)}
        for name, cells in lists.items():
            recs, planes = m.catchments(cells, drop=True)
            own = planes["drop"][np.isfinite(planes["drop"])]
            bh = float(own.max()) / BINS if own.size and own.max() > 0 else 1.0
            row["lists"][name] = {"gauges": len(cells), "gauged_cells": sum(r["cells"] for r in recs), "largest_own": max(r["cells"] for r in recs),
                                  "largest_area": max(r["area"] for r in recs), "steps_max": max(r["steps_max"] for r in recs), "bin_height": bh}
            del recs, planes
            fs[name + "/records"] = c_catchments(m, cells, 0, 0.0, ())
            fs[name + "/bins32"] = c_catchments(m, cells, BINS, bh, ())
            if not a.trace_calls:
                fs[name + "/all_planes"] = c_catchments(m, cells, 0, 0.0, PLANES)
        if a.trace_calls:
            for k, f in fs.items():
                if k != "flowpaths_records":
                    for _ in range(a.trace_calls):
                        f()
            row["traced_calls"] = a.trace_calls
            rec["states"].append(row)
            continue
        for f in fs.values():
            for _ in range(a.warmup):
                f()
        wall = {k: [] for k in fs}
        for _ in range(a.calls):            # the calls in turns, so that whatever else the machine does meets them alike
            for k, f in fs.items():
                t0 = time.perf_counter()
                f()
                wall[k].append(1e3 * (time.perf_counter() - t0))
        for k, w in wall.items():
            t = {"wall_ms": round(statistics.median(w), 4), "wall_ms_min": round(min(w), 4), "wall_ms_max": round(max(w), 4)}
            if "/" in k:
                row["lists"][k.split("/")[0]][k.split("/")[1]] = t
            else:
                row[k] = t
        rec["states"].append(row)
        print(f"[catchments] {n}^2 after {ticks:3d} ticks {nb:9d} basins  drainage_labels {row['drainage_labels']['wall_ms']:.3f} ms  " +
              "  ".join(f"{k} {v['records']['wall_ms']:.3f} ms" for k, v in row["lists"].items()) + " (records only, wall clock)", file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    if not a.trace_calls:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"r24_catchments_{a.tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, f"r24_catchments_{a.tag}.md"), "w") as f:
            f.write(markdown(rec) + "\n")


if __name__ == "__main__":
    main()
