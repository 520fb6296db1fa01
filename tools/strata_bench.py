#!/usr/bin/env python3
"""The strata readers (smx_soil_totals / smx_ensemble_soil_totals / smx_soil_thickness / smx_cores) timed on the device. Prints one JSON
line and writes profiles/r12_strata_<tag>.json.

usage: strata_bench.py [--sizes 1024] [--ticks 25] [--calls 10] [--warmup 3] [--members 64,256] [--no-ensemble] [--no-host] [--lib PATH]
                       [--tag bench] [--out profiles]

Per size, `rockgravelpebblessand.soil` on the relaxed engine with bench.py's area-scaled particle counts, after `ticks` ticks (deep
columns). Timed, each as the median (min, max) of `calls` after `warmup` calls (the first allocates the scratch), with HIP events on the
context's stream around the blocking call and the wall clock around it:
  totals      Layermap.soil_totals()                                  one smx_soil_totals call
  thickness   Layermap.soil_thickness([1, 2, 3, 4])                   one plane per type
  thickness3  ... with cover and sections                             three planes per type
  cores_line  Layermap.transect of the map's main diagonal            two smx_cores calls: the count, the fetch
  cores_64k   Layermap.cores of 65536 drawn cells                     likewise
The baseline is what a caller had before these entry points: Layermap.snapshot() (smx_export_columns: the whole pool crosses the host)
and the vectorised numpy fold of tests/strata_ref.py (totals_np), wall clock, `calls // 3` times; the totals must agree. The ensemble
lines: `members` maps of 256^2 `default.soil` after 10 ticks, Ensemble.soil_totals(nsoils) against the same totals member by member and
against export + fold member by member. --lib: another build of the library (an experiment build with wider workgroups)."""
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

SOIL = "rockgravelpebblessand.soil"


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


def wall(fn, calls: int) -> dict:
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"wall_ms": round(statistics.median(t), 3), "wall_ms_min": round(min(t), 3), "wall_ms_max": round(max(t), 3), "calls": calls}


def same_totals(a, b) -> bool:
    keys = ("sections", "cells", "top_cells", "volume_q40", "held_q40", "flags")
    return len(a) == len(b) and all(int(x[k]) == int(y[k]) for x, y in zip(a, b) for k in keys)


def run_size(n: int, ticks: int, calls: int, warmup: int, host: bool) -> dict:
    import strata_ref
    from soilmachine_amd.machine import Layermap
    from soilmachine_amd.soilfile import loadsoil
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    area = (n / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    nt = len(cfg.soils)
    recs, other = m.soil_totals(other=True)
    ns = m.soil_thickness(list(range(min(nt, 8))), sections=True)[1]
    depth = ns.sum(axis=0)
    out = {"size": n, "nwater": nwater, "nwind": nwind, "ticks": ticks, "pool": m.pool, "sections": int(sum(r["sections"] for r in recs) + other),
           "max_depth": int(depth.max()), "median_depth": float(np.median(depth)), "types": nt}
    rng = np.random.default_rng(1)
    drawn = rng.integers(0, n * n, size=65536).astype(np.uint32)
    out["totals"] = timed(m, lambda: m.soil_totals(), calls, warmup)
    out["thickness"] = timed(m, lambda: m.soil_thickness([1, 2, 3, 4]), calls, warmup)
    out["thickness3"] = timed(m, lambda: m.soil_thickness([1, 2, 3, 4], cover=True, sections=True), calls, warmup)
    out["cores_line"] = timed(m, lambda: m.transect((0, 0), (n - 1, n - 1)), calls, warmup)
    out["cores_64k"] = timed(m, lambda: m.cores(drawn), calls, warmup)
    out["cores_64k_sections"] = int(m.cores(drawn)[0].sum())
    if host:
        k = max(1, calls // 3)
        snap = m.snapshot()
        if not same_totals(strata_ref.totals_np(snap, nt)[0], recs):
            raise SystemExit(f"{n}^2: the device totals and the fold of the exported map DISAGREE")
        out["baseline_export"] = wall(m.snapshot, k)
        out["baseline_fold"] = wall(lambda: strata_ref.totals_np(snap, nt), k)
        base = out["baseline_export"]["wall_ms"] + out["baseline_fold"]["wall_ms"]
        out["baseline_ms"] = round(base, 3)
        out["agrees_with_the_fold"] = True
        for name in ("totals", "thickness", "thickness3", "cores_line", "cores_64k"):
            out[name]["baseline_over_call"] = round(base / out[name]["wall_ms"], 2)
            out[name]["export_over_call"] = round(out["baseline_export"]["wall_ms"] / out[name]["wall_ms"], 2)
    m.close()
    return out


def run_ensemble(members: int, calls: int, warmup: int, host: bool) -> dict:
    import strata_ref
    from soilmachine_amd.ensemble import Ensemble
    from soilmachine_amd.soilfile import loadsoil
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", "default.soil"))
    nt = len(cfg.soils)
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, 256, 256, seed=s, pool=8 * 256 * 256) for s in range(members)]
        ens.tick(250, 250, n=10)
        ens.sync()
        one = ens.soil_totals(nt)
        if not all(same_totals(a, m.soil_totals(nt)) for a, m in zip(one, mem)):
            raise SystemExit("Ensemble.soil_totals() and the member-by-member totals DISAGREE")
        row = {"members": members, "size": 256, "soil": "default.soil", "ticks": 10, "types": nt, "sections": int(sum(r["sections"] for a in one for r in a)),
               "ensemble_call": timed(mem[0], lambda: ens.soil_totals(nt), calls, warmup),
               "member_by_member": timed(mem[0], lambda: [m.soil_totals(nt) for m in mem], max(3, calls // 3), 1)}
        row["member_by_member_over_call"] = round(row["member_by_member"]["wall_ms"] / row["ensemble_call"]["wall_ms"], 2)
        if host:
            if not all(same_totals(strata_ref.totals_np(m.snapshot(), nt)[0], a) for a, m in zip(one[:4], mem[:4])):
                raise SystemExit("the ensemble totals and the fold of the exported members DISAGREE")
            row["baseline_export_fold"] = wall(lambda: [strata_ref.totals_np(m.snapshot(), nt) for m in mem], 1)
            row["baseline_over_call"] = round(row["baseline_export_fold"]["wall_ms"] / row["ensemble_call"]["wall_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024")
    ap.add_argument("--ticks", type=int, default=25)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", default="64,256")
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    rec = {"soil": SOIL, "engine": "relaxed", "calls": a.calls, "warmup_calls": a.warmup, "library": os.path.relpath(capi.LIB_PATH, ROOT), "maps": [], "ensembles": []}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        r = run_size(n, a.ticks, a.calls, a.warmup, host=not a.no_host)
        rec["maps"].append(r)
        for name in ("totals", "thickness", "thickness3", "cores_line", "cores_64k"):
            print(f"[strata] {n}^2 {name:11s} {r[name]['event_ms']:10.3f} ms (events) {r[name]['wall_ms']:10.3f} ms (wall)   baseline {r.get('baseline_ms', float('nan')):10.1f} ms",
                  file=sys.stderr, flush=True)
    if not a.no_ensemble:
        for k in [int(x) for x in a.members.split(",") if x]:
            e = run_ensemble(k, a.calls, a.warmup, host=not a.no_host)
            rec["ensembles"].append(e)
            print(f"[strata] {k} x 256^2: one call {e['ensemble_call']['wall_ms']:.3f} ms, member by member {e['member_by_member']['wall_ms']:.3f} ms, "
                  f"export + fold {e.get('baseline_export_fold', {}).get('wall_ms', float('nan')):.1f} ms", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r12_strata_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
