#!/usr/bin/env python3
"""The lake census (smx_lakes / smx_ensemble_lakes) timed on the device. Prints one JSON line and writes profiles/r11_lakes_<tag>.json.

usage: lakes_bench.py [--sizes 1024,4096] [--ticks 25] [--calls 10] [--warmup 3] [--members 256] [--no-ensemble] [--no-host] [--tag bench] [--out profiles]

Per size, `rockgravelpebblessand.soil` on the relaxed engine with bench.py's area-scaled particle counts, three states in one context:
  ticked   after `ticks` ticks
  all_wet  every cell one rock section as high as the ticked map, 0.25 of water on top: ONE lake covering the map, the worst case for
           the record's atomics
  dry      the same without the water: no lake
A census = Layermap.lakes() with cap = the lake count known from a first call (one smx_lakes call: table upload, five launches and
the scan, the results back). Times: HIP events on the context's stream around the blocking call, and the wall clock around it;
`warmup` calls first (the first one allocates the scratch), then the median (min, max) of `calls`. Achieved bytes per second are
the algorithmic bytes over the event time: per cell the 32-byte top record read twice (the wet test of k_lake_tiles, the figures
of k_lake_stats) and seven words of label-plane traffic (tiles write A; flatten reads it; the scan reads A and writes B; stats
reads A and B and writes A) = 92 bytes. The ensemble line: `members` maps of 256^2 `default.soil` after 10 ticks, Ensemble.lakes()
(two calls: count, fetch) against the same census member by member. The host path a caller had before this entry point existed:
Layermap.snapshot() and a flood fill over the exported columns (tests/lakes_ref.py), at the first size."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from soilmachine_amd import capi                       # noqa: E402
from soilmachine_amd.ensemble import Ensemble          # noqa: E402
from soilmachine_amd.machine import Layermap           # noqa: E402
from soilmachine_amd.snapshot import Snapshot          # noqa: E402
from soilmachine_amd.soilfile import loadsoil          # noqa: E402

SOIL = "rockgravelpebblessand.soil"
BYTES_PER_CELL = 2 * 32 + 7 * 4
STREAM_TBS = 5.4          # what the project's own streaming kernels reach (k_map_frequency 5.5, k_lbm_step 5.3 TB/s)


def timed(stream_of, fn, calls: int, warmup: int) -> dict:
    """fn() `warmup` + `calls` times; HIP events on the stream of `stream_of` and the wall clock around each timed call."""
    import torch
    st = torch.cuda.ExternalStream(stream_of.L.smx_stream(stream_of.h))
    for _ in range(warmup):
        fn()
    ev, wall = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(a.elapsed_time(b))
    return {"event_ms": round(statistics.median(ev), 4), "event_ms_min": round(min(ev), 4), "event_ms_max": round(max(ev), 4),
            "wall_ms": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}


def flat_snapshot(like: Snapshot, rock: np.ndarray, water: float | None) -> Snapshot:
    """Every cell one rock section of size rock[c]; `water` not None: that much Air on top of every cell."""
    n = rock.size
    if water is None:
        count = np.ones(n, np.uint32); ty = np.ones(n, np.uint32); size = rock.astype(np.float64); floor = np.zeros(n)
    else:
        count = np.full(n, 2, np.uint32)
        ty = np.tile(np.array([1, 0], np.uint32), n)
        size = np.empty(2 * n); size[0::2] = rock; size[1::2] = water
        floor = np.zeros(2 * n); floor[1::2] = rock
    z = np.zeros(n, np.float32)
    return Snapshot(like.dimx, like.dimy, like.scale, like.nsoils, 0, 0, count, ty, size, floor, np.zeros(size.size), z, z.copy(), z.copy())


def census_row(m: Layermap, state: str, calls: int, warmup: int) -> dict:
    cells = m.dimx * m.dimy
    recs = m.lakes()
    n = len(recs)
    row = {"state": state, "lakes": n, "wet_cells": int(sum(r["cells"] for r in recs)), "largest_lake": max((r["cells"] for r in recs), default=0)}
    row.update(timed(m, lambda: m.lakes(cap=n), calls, warmup))
    row["count_only"] = timed(m, lambda: m.lakes(cap=0), calls, 1)
    gb = cells * BYTES_PER_CELL / 1e9
    row["algorithmic_gb"] = round(gb, 4)
    row["gb_per_s"] = round(gb / (row["event_ms"] / 1e3), 1)
    row["share_of_stream_rate"] = round(row["gb_per_s"] / (1e3 * STREAM_TBS), 4)
    return row


def run_size(n: int, ticks: int, calls: int, warmup: int, host: bool) -> dict:
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    area = (n / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    out = {"size": n, "nwater": nwater, "nwind": nwind, "ticks": ticks, "states": [census_row(m, "ticked", calls, warmup)]}
    fig = {"heights": m.heights()}
    if host:
        import lakes_ref
        t0 = time.perf_counter()
        snap = m.snapshot()
        t1 = time.perf_counter()
        want = lakes_ref.census(snap)
        t2 = time.perf_counter()
        got = m.lakes(labels=True)
        lakes_ref.assert_same_census(got, want, f"{n}^2 ticked")
        out["host_path"] = {"snapshot_s": round(t1 - t0, 3), "flood_fill_s": round(t2 - t1, 3), "total_s": round(t2 - t0, 3), "sections": snap.nsec,
                            "agrees_with_the_device": True}
        like = snap
    else:
        like = Snapshot(n, n, cfg.SCALE, len(cfg.soils), 0, 0, None, None, None, None, None, None, None, None)
    for state, water in (("all_wet", 0.25), ("dry", None)):
        m.load(flat_snapshot(like, fig["heights"], water))
        out["states"].append(census_row(m, state, calls, warmup))
    m.close()
    return out


def run_ensemble(members: int, calls: int, warmup: int) -> dict:
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", "default.soil"))
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, 256, 256, seed=s, pool=8 * 256 * 256) for s in range(members)]
        ens.tick(250, 250, n=10)
        ens.sync()
        one = ens.lakes()
        each = [m.lakes() for m in mem]
        if one != each:
            raise SystemExit("Ensemble.lakes() and the member-by-member census DISAGREE")
        row = {"members": members, "size": 256, "soil": "default.soil", "ticks": 10, "lakes_total": sum(len(x) for x in one),
               "ensemble_call": timed(mem[0], ens.lakes, calls, warmup), "member_by_member": timed(mem[0], lambda: [m.lakes() for m in mem], max(3, calls // 3), 1)}
        row["speedup_wall"] = round(row["member_by_member"]["wall_ms"] / row["ensemble_call"]["wall_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--ticks", type=int, default=25)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    rec = {"soil": SOIL, "engine": "relaxed", "bytes_per_cell": BYTES_PER_CELL, "stream_rate_tb_s": STREAM_TBS, "calls": a.calls, "warmup_calls": a.warmup, "maps": []}
    for i, n in enumerate(sizes):
        r = run_size(n, a.ticks, a.calls, a.warmup, host=(i == 0 and not a.no_host))
        rec["maps"].append(r)
        for s in r["states"]:
            print(f"[lakes] {n}^2 {s['state']:8s} {s['lakes']:7d} lakes  {s['event_ms']:9.3f} ms (events)  {s['wall_ms']:9.3f} ms (wall)  {s['gb_per_s']:8.1f} GB/s", file=sys.stderr, flush=True)
    if not a.no_ensemble:
        rec["ensemble"] = run_ensemble(a.members, a.calls, a.warmup)
        e = rec["ensemble"]
        print(f"[lakes] {e['members']} x 256^2: one call {e['ensemble_call']['wall_ms']:.3f} ms, member by member {e['member_by_member']['wall_ms']:.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r11_lakes_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
