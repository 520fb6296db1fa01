#!/usr/bin/env python3
"""The horizons (smx_horizons) timed on the device. Prints one JSON line and writes <out>/r25_horizons_<tag>.json and
<out>/r25_horizons_<tag>.md, the tables of profiles/r25_horizons.md.

usage: horizons_bench.py [--size 4096] [--ticks 0,20] [--calls 5] [--warmup 2] [--trace-calls 0] [--lib PATH] [--tag bench] [--out profiles]
       horizons_bench.py --split <dir>
       horizons_bench.py --probes [--size 512] [--ticks 0,20]

A `rockgravelpebblessand.soil` map of size^2, on the initial terrain (ticks 0) and spun up on the relaxed engine with bench.py's
area-scaled particle counts (ticks 20). In the same run, on the same state, through ctypes into buffers made once (the C-ABI's own
cost, no Python record), for 1, 8 and 16 directions (masks 0x0001, 0x5555, 0xFFFF) and reach 0 and 64:
  records      smx_horizons, no plane, no sun
  sky          the same with the sky plane: the slopes and steps of all directions kept in scratch, k_horizon_sky, one plane copied back
  all_planes   slope, step, sky, open and lit with one sun: nd * 12 + 16 bytes per cell copied to the host
and beside them, once per state:
  drainage_labels     smx_drainage with cap = the basin count and the label plane: the yardstick among the siblings
Times: the wall clock around the blocking call (it ends in its one synchronisation, with the results on the host, and starts on an
idle stream); `warmup` calls of each first (the first one allocates the scratch), then `calls` rounds of all of them in turns: the
median (min, max) of each.

The second yardstick is the same scan with the tile levels switched off, a compile-time switch of a bench build that is no product:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -DSMX_HORIZON_NO_TILES -o build/libsoilmx_notiles.so soilmachine_amd/csrc/soilmx.hip
  python tools/horizons_bench.py --lib build/libsoilmx_notiles.so --tag walk
(--lib: the library to load instead of the package's own.) Per-kernel times come from a run of their own under the profiler:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/horizons_bench.py --trace-calls 3
  python tools/horizons_bench.py --split <dir>
With --trace-calls N the timed section is replaced by N records-only calls per mask, reach and state, in the order of the table, so
--split can tell them apart by their position: the mean duration of k_horizon_heights and k_horizon_scan of every one of them.

--probes needs no device beyond the spin-up: the state is snapshotted and the host build of the same bodies (tests/horizons_host)
counts, per ray, the tile bounds it computes and the heights it loads, beside the steps the plain walk takes."""
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
MASKS = (("1", 0x0001), ("8", 0x5555), ("16", 0xFFFF))
REACHES = (0, 64)
KINDS = ("records", "sky", "all_planes")
KERNELS = ("k_horizon_heights", "k_horizon_scan", "k_horizon_sky")


def c_horizons(m, mask: int, reach: int, kind: str):
    from soilmachine_amd import capi
    nd, n = bin(mask).count("1"), m.dimx * m.dimy
    out = (capi.Horizon * nd)()
    want = {"records": (), "sky": ("sky",), "all_planes": ("slope", "step", "sky", "open", "lit")}[kind]
    sizes = {"slope": (np.float64, nd * n), "step": (np.uint32, nd * n), "sky": (np.float64, n), "open": (np.uint32, n), "lit": (np.uint32, n)}
    buf = {k: np.zeros(sizes[k][1], sizes[k][0]) for k in want}
    suns = capi.horizon_suns([(0, 0.25)]) if "lit" in want else None
    counts = np.zeros(1, np.uint32)
    args = [capi.ptr(buf.get(k)) for k in ("slope", "step", "sky", "open", "lit")]
    return lambda: m._chk(m.L.smx_horizons(m.h, mask, reach, out, C.sizeof(capi.Horizon), suns, 1 if suns is not None else 0, capi.ptr(counts) if suns is not None else None, *args))


def c_drainage_labels(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    labels = np.zeros(m.dimx * m.dimy, np.uint32)
    return lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, capi.ptr(labels), None))


def split(d: str, states: int) -> dict:
    """The per-dispatch kernel trace under `d` -> per state, mask and reach (the order --trace-calls queued them in): the mean
    duration (ms) of the heights and the scan kernel of one call."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + d)
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    got = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if k in r["Kernel_Name"]] for k in KERNELS[:2]}
    slots = states * len(MASKS) * len(REACHES)                 # (--trace-calls queues nothing but `per` calls of each, in this order)
    per = len(got["k_horizon_scan"]) // slots if slots else 0
    out, at = [], 0
    for s in range(states):
        for name, _ in MASKS:
            for reach in REACHES:
                seg = {k: got[k][at:at + per] for k in got}
                out.append({"state": s, "directions": name, "reach": reach, "calls": per, **{k + "_ms": round(statistics.mean(v), 4) for k, v in seg.items() if v}})
                at += per
    return {"per_call": out}


def markdown(rec: dict) -> str:
    """The timing tables of a run."""
    out = [f"## {rec['size']}^2 `{rec['soil']}`, relaxed engine, library `{rec['lib']}`, median (min .. max) of {rec['calls']} calls, wall clock in ms", ""]
    for st in rec["states"]:
        y = st["drainage_labels"]
        out += [f"### after {st['ticks']} ticks", "", f"`smx_drainage` with the label plane: {y['wall_ms']:.3f} ({y['wall_ms_min']:.3f} .. {y['wall_ms_max']:.3f})", "",
                "| directions | reach | bounded cells | largest step | records | sky | all planes |", "|---|---|---|---|---|---|---|"]
        for key, row in st["configs"].items():
            f = lambda k: f"{row[k]['wall_ms']:.3f} ({row[k]['wall_ms_min']:.3f} .. {row[k]['wall_ms_max']:.3f})" if k in row else "-"
            out.append(f"| {row['directions']} | {row['reach']} | {row['bounded']} | {row['step_max']} | {f('records')} | {f('sky')} | {f('all_planes')} |")
        out.append("")
    return "\n".join(out)


def probes(a, m, ticks: int) -> dict:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from horizons_host_lib import horizons as H, horizons_no_tiles as HN
    s = m.snapshot()
    row = {"ticks": ticks, "configs": {}}
    for name, mask in MASKS:
        for reach in REACHES:
            rays, bounds, loads = H.run(s, mask, reach, planes=())[3]
            _, _, steps = HN.run(s, mask, reach, planes=())[3]
            row["configs"][f"{name}/{reach}"] = {"rays": rays, "bounds_per_ray": round(bounds / rays, 3), "loads_per_ray": round(loads / rays, 3), "walk_steps_per_ray": round(steps / rays, 3)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--ticks", default="0,20")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--split", default="")
    ap.add_argument("--probes", action="store_true")
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
    n = a.size or (512 if a.probes else 4096)
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
        if a.probes:
            rec["states"].append(probes(a, m, ticks))
            continue
        row = {"ticks": ticks, "configs": {}}
        fs = {}
        if not a.trace_calls:
            nb = C.c_uint32()
            m._chk(m.L.smx_drainage(m.h, None, C.sizeof(capi.Basin), 0, C.byref(nb), None, None, None))
            fs["drainage_labels"] = c_drainage_labels(m, int(nb.value))
        for name, mask in MASKS:
            for reach in REACHES:
                key = f"{name}/{reach}"
                row["configs"][key] = {"directions": int(name), "reach": reach}
                for kind in (("records",) if a.trace_calls else kinds):
                    fs[f"{key}/{kind}"] = c_horizons(m, mask, reach, kind)
        if a.trace_calls:
            for f in fs.values():
                for _ in range(a.trace_calls):
                    f()
            row["traced_calls"] = a.trace_calls
            rec["states"].append(row)
            continue
        for key, c in row["configs"].items():                  # what the calls find (the first call of each shape allocates its scratch)
            recs = m.horizons(dict(MASKS)[str(c["directions"])], c["reach"])
            c["bounded"], c["step_max"], c["step_sum"] = sum(r["bounded"] for r in recs), max(r["step_max"] for r in recs), sum(r["step_sum"] for r in recs)
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
        print(f"[horizons] {n}^2 after {ticks:3d} ticks  drainage_labels {row['drainage_labels']['wall_ms']:.3f} ms  " +
              "  ".join(f"{k} {v['records']['wall_ms']:.3f} ms" for k, v in row["configs"].items() if "records" in v) + " (records only, wall clock)", file=sys.stderr, flush=True)
    m.close()
    print(json.dumps(rec), flush=True)
    if not a.trace_calls:
        os.makedirs(a.out, exist_ok=True)
        tag = a.tag + ("_probes" if a.probes else "")
        with open(os.path.join(a.out, f"r25_horizons_{tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        if not a.probes:
            with open(os.path.join(a.out, f"r25_horizons_{tag}.md"), "w") as f:
                f.write(markdown(rec) + "\n")


if __name__ == "__main__":
    main()
