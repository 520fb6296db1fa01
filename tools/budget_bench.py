#!/usr/bin/env python3
"""The sediment budget (smx_budget / smx_ensemble_budget) timed on the device. Prints one JSON line and writes
<out>/r23_budget_<tag>.json.

usage: budget_bench.py [--size 4096] [--fork 5] [--ticks 25] [--calls 10] [--warmup 3] [--members 64] [--no-ensemble] [--no-host]
                       [--trace-calls 0] [--tag bench] [--out profiles]
       budget_bench.py --split <dir>

A `rockgravelpebblessand.soil` map of size^2 on the relaxed engine with bench.py's area-scaled particle counts: at tick `fork` its
state is kept in a second map (Layermap.copy_from), at tick `ticks` the two are compared. In the same run, on the same two states,
through ctypes into buffers made once (the C-ABI's own cost, no Python record), each as the median (min, max) of `calls` after
`warmup` calls (the first allocates the scratch), with HIP events on the context's stream around the blocking call and the wall clock
around it:
  budget_records    smx_budget with cap = the basin count known from a first call, no soil table, no plane
  budget_soils      the same with the soil table
  budget_planes     the same with the soil table and all four planes: four 64-bit plane copies to the host
What it is made of, as yardsticks:
  drainage_labels   smx_drainage on the base with cap = the basin count and the label plane
  totals_base / totals_now   smx_soil_totals on each map
What a caller had before, wall clock, `calls // 3` times: two Layermap.snapshot() calls and the vectorised numpy fold of
tests/budget_ref.py (budget_np, given the label plane); its integers must agree with the device's.
The ensemble line: `members` maps of 256^2 `default.soil` forked from one spun-up source (10 ticks) with different seeds and ticked
twice, Ensemble.budget(source) against the same budgets member by member.

Per-kernel times come from a run of their own under the profiler, which then holds nothing but the calls to be split up:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/budget_bench.py --trace-calls 3
  python tools/budget_bench.py --split <dir>
With --trace-calls N the timed section is replaced by N budget_soils calls, N smx_soil_totals calls on each map and N
drainage_labels calls. --split reads the per-dispatch trace: the dispatches and the total, mean, min and max duration of
k_budget_fold, k_budget_where, k_strata_totals and the chain's kernels."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SOIL = "rockgravelpebblessand.soil"
PLANES = (("dground", np.float64), ("dheight", np.float64), ("dsolid", np.int64), ("dwater", np.int64))
KERNELS = ("k_budget_fold", "k_budget_where", "k_strata_totals", "k_drain_stats", "k_drain_resolve", "k_drain_recv", "k_lake_tiles", "k_lake_merge", "k_lake_flatten")


def timed(stream_of, fn, calls: int, warmup: int) -> dict:
    """fn() `warmup` + `calls` times; HIP events on the stream of `stream_of` and the wall clock around each timed call."""
    hip = C.CDLL("libamdhip64.so")               # (the runtime the library itself is linked against: its events, on the library's stream)
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    st = C.c_void_p(stream_of.L.smx_stream(stream_of.h))
    a, b, ms = C.c_void_p(), C.c_void_p(), C.c_float()
    if hip.hipEventCreate(C.byref(a)) or hip.hipEventCreate(C.byref(b)):
        raise SystemExit("hipEventCreate failed")
    for _ in range(warmup):
        fn()
    ev, wall = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        hip.hipEventRecord(a, st)
        fn()
        hip.hipEventRecord(b, st)
        hip.hipEventSynchronize(b)
        wall.append(1e3 * (time.perf_counter() - t0))
        if hip.hipEventElapsedTime(C.byref(ms), a, b):
            raise SystemExit("hipEventElapsedTime failed")
        ev.append(ms.value)
    hip.hipEventDestroy(a); hip.hipEventDestroy(b)
    return {"event_ms": round(statistics.median(ev), 4), "event_ms_min": round(min(ev), 4), "event_ms_max": round(max(ev), 4),
            "wall_ms": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}


def wall(fn, calls: int) -> dict:
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"wall_ms": round(statistics.median(t), 3), "wall_ms_min": round(min(t), 3), "wall_ms_max": round(max(t), 3), "calls": calls}


def c_budget(m, base, cap: int, ntypes: int, planes: bool):
    """(call, basin records, soil records, plane buffers) of one smx_budget shape"""
    from soilmachine_amd import capi
    out = (capi.BudgetBasin * max(1, cap))()
    soils = (capi.BudgetSoil * max(1, ntypes))() if ntypes else None
    n = C.c_uint32()
    buf = {k: np.zeros(m.dimx * m.dimy, dt) for k, dt in PLANES} if planes else {}
    args = [capi.ptr(buf.get(k)) for k, _ in PLANES]
    return (lambda: m._chk(m.L.smx_budget(m.h, base.h, out, C.sizeof(capi.BudgetBasin), cap, C.byref(n), soils, C.sizeof(capi.BudgetSoil), ntypes, *args))), out, soils, buf


def c_drainage_labels(m, cap: int):
    from soilmachine_amd import capi
    out = (capi.Basin * max(1, cap))()
    n = C.c_uint32()
    labels = np.zeros(m.dimx * m.dimy, np.uint32)
    return (lambda: m._chk(m.L.smx_drainage(m.h, out, C.sizeof(capi.Basin), cap, C.byref(n), None, capi.ptr(labels), None))), labels


def c_totals(m, ntypes: int):
    from soilmachine_amd import capi
    out = (capi.SoilTotal * ntypes)()
    return lambda: m._chk(m.L.smx_soil_totals(m.h, out, C.sizeof(capi.SoilTotal), ntypes, None))


def split(d: str) -> dict:
    """The per-dispatch kernel trace under `d` -> per kernel of KERNELS: the dispatches and the total, mean, min and max duration (ms)."""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + d)
    got = {k: [] for k in KERNELS}
    for r in csv.DictReader(open(f[0])):
        kind = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if kind:
            got[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return {k: {"n": len(v), "total_ms": round(sum(v), 3), "mean_ms": round(statistics.mean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in got.items() if v}


def run_map(a) -> dict:
    import budget_ref
    from soilmachine_amd import capi
    from soilmachine_amd.machine import Layermap
    from soilmachine_amd.soilfile import loadsoil
    n = a.size
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    area = (n / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    m = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED)
    base = Layermap(cfg, n, n, seed=0, engine=capi.ENGINE_RELAXED, initialize=False)
    for _ in range(a.fork):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    base.copy_from(m)
    for _ in range(a.ticks - a.fork):
        m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()
    nt = len(cfg.soils)
    nb = C.c_uint32()
    m._chk(m.L.smx_budget(m.h, base.h, None, C.sizeof(capi.BudgetBasin), 0, C.byref(nb), None, 0, 0, None, None, None, None))
    nb = int(nb.value)
    out = {"size": n, "soil": SOIL, "engine": "relaxed", "nwater": nwater, "nwind": nwind, "fork_tick": a.fork, "ticks": a.ticks, "types": nt, "basins": nb,
           "sections_base": base.digest()["nsec"], "sections_now": m.digest()["nsec"]}
    records, soils, planes = c_budget(m, base, nb, 0, False), c_budget(m, base, nb, nt, False), c_budget(m, base, nb, nt, True)
    drain, labels = c_drainage_labels(base, nb)
    tb, tn = c_totals(base, nt), c_totals(m, nt)
    if a.trace_calls:
        for f in (soils[0], tb, tn, drain):
            for _ in range(a.trace_calls):
                f()
        out["traced_calls"] = a.trace_calls
        return out
    out["budget_records"] = timed(m, records[0], a.calls, a.warmup)
    out["budget_soils"] = timed(m, soils[0], a.calls, a.warmup)
    out["budget_planes"] = timed(m, planes[0], a.calls, a.warmup)
    out["drainage_labels"] = timed(base, drain, a.calls, a.warmup)
    out["totals_base"] = timed(base, tb, a.calls, a.warmup)
    out["totals_now"] = timed(m, tn, a.calls, a.warmup)
    recs = [soils[1][k].as_dict() for k in range(nb)]
    table = [soils[2][t].as_dict() for t in range(nt)]
    dg = planes[3]["dground"]
    out.update(lowered_cells=sum(r["lowered_cells"] for r in recs), raised_cells=sum(r["raised_cells"] for r in recs), resurfaced_cells=sum(r["resurfaced_cells"] for r in recs),
               eroded=sum(r["eroded"] for r in recs), deposited=sum(r["deposited"] for r in recs), cut_max=max(r["cut_max"] for r in recs), fill_max=max(r["fill_max"] for r in recs),
               flags=int(np.bitwise_or.reduce([r["flags"] for r in recs])), soils=[{k: q[k] for k in ("gained", "lost", "surfaced", "covered")} for q in table])
    if int((dg < 0).sum()) != out["lowered_cells"] or int((dg > 0).sum()) != out["raised_cells"]:
        raise SystemExit("the dground plane and the records DISAGREE")
    if not a.no_host:
        k = max(1, a.calls // 3)
        sb, sn = base.snapshot(), m.snapshot()
        lab = labels.reshape(n, n)
        np_b, np_s = budget_ref.budget_np(sb, sn, lab, nt)
        if [int(v) for v in np_b["eroded_q40"]] != [r["eroded_q40"] for r in recs] or [int(v) for v in np_b["lowered_cells"]] != [r["lowered_cells"] for r in recs] or \
                [(q["gained_q40"], q["lost_q40"]) for q in np_s] != [(q["gained_q40"], q["lost_q40"]) for q in table]:
            raise SystemExit("the device budget and the fold of the two exported maps DISAGREE")
        out["agrees_with_the_fold"] = True
        out["baseline_export_base"] = wall(base.snapshot, k)
        out["baseline_export_now"] = wall(m.snapshot, k)
        out["baseline_fold"] = wall(lambda: budget_ref.budget_np(sb, sn, lab, nt), k)
        out["baseline_ms"] = round(out["baseline_export_base"]["wall_ms"] + out["baseline_export_now"]["wall_ms"] + out["baseline_fold"]["wall_ms"], 3)
        for name in ("budget_records", "budget_soils", "budget_planes"):
            out[name]["baseline_over_call"] = round(out["baseline_ms"] / out[name]["wall_ms"], 2)
    m.close(); base.close()
    return out


def run_ensemble(members: int, calls: int, warmup: int) -> dict:
    from soilmachine_amd.ensemble import Ensemble
    from soilmachine_amd.machine import Layermap
    from soilmachine_amd.soilfile import loadsoil
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", "default.soil"))
    nt = len(cfg.soils)
    src = Layermap(cfg, 256, 256, seed=0, pool=8 * 256 * 256)
    for _ in range(10):
        src._chk(src.L.smx_tick(src.h, 250, 250, 1, 1))
    src.sync()
    with Ensemble(0) as ens:
        mem = ens.fork(src, members, seeds=list(range(1, members + 1)), pool=8 * 256 * 256)
        ens.tick(250, 250, n=2)
        ens.sync()
        one = ens.budget(src, nt)
        if [str(x) for x in one[:4]] != [str(m.budget(src, nt)) for m in mem[:4]]:
            raise SystemExit("Ensemble.budget() and the member-by-member budgets DISAGREE")
        row = {"members": members, "size": 256, "soil": "default.soil", "source_ticks": 10, "member_ticks": 2, "types": nt, "basins": len(one[0][0]),
               "ensemble_call": timed(mem[0], lambda: ens.budget(src, nt), calls, warmup),
               "member_by_member": timed(mem[0], lambda: [m.budget(src, nt) for m in mem], max(3, calls // 3), 1)}
        row["member_by_member_over_call"] = round(row["member_by_member"]["wall_ms"] / row["ensemble_call"]["wall_ms"], 2)
    src.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--fork", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=25)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--split", default="")
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.split:
        print(json.dumps({"kernels": split(a.split)}), flush=True)
        return
    rec = {"calls": a.calls, "warmup_calls": a.warmup, "map": run_map(a)}
    r = rec["map"]
    for name in ("budget_records", "budget_soils", "budget_planes", "drainage_labels", "totals_base", "totals_now"):
        if name in r:
            print(f"[budget] {a.size}^2 {name:16s} {r[name]['event_ms']:10.3f} ms (events) {r[name]['wall_ms']:10.3f} ms (wall)   baseline {r.get('baseline_ms', float('nan')):10.1f} ms",
                  file=sys.stderr, flush=True)
    if not a.no_ensemble and not a.trace_calls:
        e = rec["ensemble"] = run_ensemble(a.members, a.calls, a.warmup)
        print(f"[budget] {a.members} x 256^2: one call {e['ensemble_call']['wall_ms']:.3f} ms, member by member {e['member_by_member']['wall_ms']:.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"r23_budget_{a.tag}.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
