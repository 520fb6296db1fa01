#!/usr/bin/env python3
"""Proximity (smx_proximity) timed on the device. Prints one JSON line and writes <out>/r26_proximity_<tag>.json and
<out>/r26_proximity_<tag>.md, the tables of profiles/r26_proximity.md.

usage: proximity_bench.py [--size 4096] [--ticks 0,20] [--calls 5] [--warmup 2] [--trace-calls 0] [--lib PATH] [--tag bench] [--out profiles]
       proximity_bench.py --split <dir>

A `rockgravelpebblessand.soil` map of size^2, on the initial terrain (ticks 0) and spun up on the relaxed engine with bench.py's
area-scaled particle counts (ticks 20). In the same run, on the same state, through ctypes into buffers made once (the C-ABI's own
cost, no Python record), for the site sets
  water      the wet cells, grouped by their lakes (cap = the lake count)
  16 / 4096 / 65536   that many distinct random cells (one seeded draw per count)
  channels   the channel cells of streams(256)
each as
  records      no plane, no bins
  bins32       32 bins of width 4
  all_planes   nearest, group and dist2: 12 bytes per cell copied to the host
and beside them, once per state, the yardsticks among the siblings:
  lakes_labels        smx_lakes with cap = the lake count and the label plane
  drainage_labels     smx_drainage with cap = the basin count and the label plane
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host, and starts on an
idle stream); `warmup` calls of each first (the first one allocates the scratch), then `calls` rounds of all of them in turns: the
median (min, max) of each.

The band count of the envelopes is a compile-time constant of the library (PROX_BANDS of soil_prox.h). The other counts are bench
builds that are no product, each timed by a run of this tool (--lib: the library to load instead of the package's own):
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -DSMX_PROX_BANDS=1 -o build/libsoilmx_bands1.so soilmachine_amd/csrc/soilmx.hip
  python tools/proximity_bench.py --lib build/libsoilmx_bands1.so --tag bands1
Per-kernel times come from a run of their own under the profiler, with no counters in it:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/proximity_bench.py --trace-calls 3
  python tools/proximity_bench.py --split <dir>
With --trace-calls N the timed section is replaced by N records-only calls per site set and state, in the order of the table, so
--split can tell them apart by their position: the mean duration of every k_prox_* kernel of each."""
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
SETS = ("water", "16", "4096", "65536", "channels")
KINDS = ("records", "bins32", "all_planes")
KERNELS = ("k_prox_mark", "k_prox_columns", "k_prox_envelope", "k_prox_query", "k_prox_hist")


def sites_of(m, which: str):
    """The list of a site set (None: water)."""
    n = m.dimx * m.dimy
    if which == "water":
        return None
    if which == "channels":
        return np.ascontiguousarray(np.flatnonzero(m.streams(256, order=True)[1]["order"].reshape(-1)), np.uint32)
    return np.ascontiguousarray(np.random.default_rng(int(which)).choice(n, size=min(n, int(which)), replace=False), np.uint32)


def c_proximity(m, cl, cap: int, kind: str):
    from soilmachine_amd import capi
    n = m.dimx * m.dimy
    out = (capi.Proximity * max(1, cap))()
    bins = 32 if kind == "bins32" else 0
    hist = np.zeros(max(1, cap * bins), np.uint32)
    buf = [np.zeros(n, np.uint32) for _ in range(3)] if kind == "all_planes" else [None] * 3
    count = C.c_uint32()
    return lambda: m._chk(m.L.smx_proximity(m.h, capi.ptr(cl), 0 if cl is None else len(cl), out if cap else None, C.sizeof(capi.Proximity), cap, C.byref(count),
                                            capi.ptr(hist) if bins else None, bins, 4, *[capi.ptr(b) for b in buf]))


def c_lakes_labels(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Lake * max(1, cap))()
    n = C.c_uint32()
    labels = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_lakes(m.h, out, C.sizeof(capi.Lake), cap, C.byref(n), capi.ptr(labels)))


def c_drainage_labels(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    labels = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, capi.ptr(labels), None))


def split(d: str, states: int) -> dict:
    """The per-dispatch kernel trace under `d` -> per state and site set (the order --trace-calls queued them in): the mean
    duration (ms) of each proximity kernel of one call."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + d)
    rows = sorted((r for name in f for r in csv.DictReader(open(name))), key=lambda r: int(r["Start_Timestamp"]))
    got = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if k in r["Kernel_Name"]] for k in KERNELS[:4]}
    slots = states * len(SETS)                                  # (--trace-calls queues nothing but `per` calls of each, in this order)
    per = len(got["k_prox_envelope"]) // slots if slots else 0
    out, at = [], 0
    for s in range(states):
        for which in SETS:
            seg = {k: got[k][at:at + per] for k in got}
            out.append({"state": s, "sites": which, "calls": per, **{k + "_ms": round(statistics.mean(v), 4) for k, v in seg.items() if v}})
            at += per
    return {"per_call": out}


def markdown(rec: dict) -> str:
    """The timing tables of a run."""
    out = [f"## {rec['size']}^2 `{rec['soil']}`, relaxed engine, median (min .. max) of {rec['calls']} calls, wall clock in ms", ""]
    for st in rec["states"]:
        f = lambda t: f"{t['wall_ms']:.3f} ({t['wall_ms_min']:.3f} .. {t['wall_ms_max']:.3f})"
        out += [f"### after {st['ticks']} ticks", "", f"`smx_lakes` with the label plane: {f(st['lakes_labels'])}; `smx_drainage` with the label plane: {f(st['drainage_labels'])}", "",
                "| sites | site cells | records | largest dist2 | records | 32 bins | all planes |", "|---|---|---|---|---|---|---|"]
        for key, row in st["configs"].items():
            out.append(f"| {key} | {row['site_cells']} | {row['nrecords']} | {row['dist2_max']} | " + " | ".join(f(row[k]) if k in row else "-" for k in KINDS) + " |")
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ticks", default="0,20")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--split", default="")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--lib", default="")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    states = [int(x) for x in a.ticks.split(",") if x]
    if a.split:
        print(json.dumps(split(a.split, len(states))), flush=True)
        return
    from soilmachine_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    from soilmachine_amd.machine import Layermap
    from soilmachine_amd.soilfile import loadsoil
    n = a.size
    kinds = [k for k in a.kinds.split(",") if k]
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    scale = (n / 256.0) ** 2
    nwater, nwind = int(250 * scale), int(250 * scale * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    rec = {"soil": SOIL, "engine": "relaxed", "size": n, "nwater": nwater, "nwind": nwind, "calls": a.calls, "warmup_calls": a.warmup,
           "lib": os.path.relpath(capi.LIB_PATH, ROOT), "states": []}
    done = 0
    for ticks in sorted(states):
        for _ in range(ticks - done):
            m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
        done = ticks
        m.sync()
        row = {"ticks": ticks, "configs": {}}
        fs = {}
        nl = C.c_uint32()
        m._chk(m.L.smx_lakes(m.h, None, C.sizeof(capi.Lake), 0, C.byref(nl), None))
        if not a.trace_calls:
            nb = C.c_uint32()
            m._chk(m.L.smx_drainage(m.h, None, C.sizeof(capi.Basin), 0, C.byref(nb), None, None, None))
            fs["lakes_labels"] = c_lakes_labels(m, int(nl.value))
            fs["drainage_labels"] = c_drainage_labels(m, int(nb.value))
        for which in SETS:
            cl = sites_of(m, which)
            if cl is not None and not len(cl):
                continue                                       # (no channel cell: nothing to list)
            cap = int(nl.value) if cl is None else len(cl)
            row["configs"][which] = {}
            if not a.trace_calls:                              # what the calls find (the first call allocates the scratch)
                recs, pl = m.proximity(cl, dist2=True)
                d2 = pl["dist2"]
                row["configs"][which] = {"site_cells": int((d2 == 0).sum()), "nrecords": len(recs), "dist2_max": int(d2.max()) if len(recs) else 0}
            for kind in (("records",) if a.trace_calls else kinds):
                fs[f"{which}/{kind}"] = c_proximity(m, cl, cap, kind)
        if a.trace_calls:
            for f in fs.values():
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
                row["configs"][k.rsplit("/", 1)[0]][k.rsplit("/", 1)[1]] = t
            else:
                row[k] = t
        rec["states"].append(row)
        cells = [v[k]["wall_ms"] for v in row["configs"].values() for k in KINDS if k in v]
        row["mean_ms"] = round(statistics.mean(cells), 4) if cells else 0.0
        print(f"[proximity] {rec['lib']} mean {row['mean_ms']:.3f} ms  {n}^2 after {ticks:3d} ticks  lakes_labels {row['lakes_labels']['wall_ms']:.3f} ms  drainage_labels {row['drainage_labels']['wall_ms']:.3f} ms  " +
              "  ".join(f"{k} {v['records']['wall_ms']:.3f} ms" for k, v in row["configs"].items() if "records" in v) + " (records only, wall clock)", file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    if not a.trace_calls:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"r26_proximity_{a.tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, f"r26_proximity_{a.tag}.md"), "w") as f:
            f.write(markdown(rec) + "\n")


if __name__ == "__main__":
    main()
