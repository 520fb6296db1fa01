#!/usr/bin/env python3
"""Ensembles of exact maps (smx_ensemble_*): the tick of B members against one standalone SERIAL context and the reference's
one-core loop. Workload: default.soil at 256^2, 250 water + 250 wind particles per tick, seeds 0..B-1, pools of 8 sections per
cell; 5 warm-up ticks, 20 timed. Prints one JSON line and writes profiles/r07_ensemble_<tag>.json.

usage: ensemble_bench.py [--batches 1,8,64,256,1024] [--warmup 5] [--ticks 20] [--tag bench] [--out profiles] [--no-record] [--no-ref]
       ensemble_bench.py --observe [--batches 1,8,64,256,1024] [--calls 10] [--tag observe]     (writes profiles/r09_ensemble_<tag>.json)

--observe: the ensemble OBSERVED in one call (smx_ensemble_figures / smx_ensemble_plane_stats) against the per-member path that
yields the same numbers on the same state (B x smx_digest + the counter / generator getters; B x smx_read_heights + the numpy member
loop), on the state after tick 25 of the same workload. Both paths must agree bit for bit before a time is printed; times are the
median wall clock of blocking calls (2 warm-up calls first).

Per B: ms per ensemble tick from device events (and its phase split), wall ms per tick, aggregate top-level water steps per second,
per-member slowdown against B = 1. Next to it: the same ticks on one standalone SERIAL context, and the reference's own loop
(oracle/_ref/soil_ref_lean, run as tools/p2_reference.py runs it, one process per core) for one member: from that, how many host
cores the ensemble is worth."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soilmachine_amd import capi                       # noqa: E402
from soilmachine_amd.ensemble import Ensemble          # noqa: E402
from soilmachine_amd.machine import Layermap           # noqa: E402
from soilmachine_amd.soilfile import loadsoil          # noqa: E402

SOIL, SIZE, NWATER, NWIND = "default.soil", 256, 250, 250
PHASES = ("ms_water", "ms_grid", "ms_wind", "ms_freq")


def _tick_ms(t: dict) -> float:
    return sum(t[k] for k in PHASES)


def run_ensemble(cfg, b: int, warmup: int, ticks: int) -> dict:
    pool = 8 * SIZE * SIZE
    t0 = time.perf_counter()
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, SIZE, SIZE, seed=s, pool=pool) for s in range(b)]
        t_add = time.perf_counter() - t0
        ens.tick(NWATER, NWIND, n=warmup)
        ens.sync()
        s0 = sum(m.counters()["steps_water_top"] for m in mem)
        ens.timing_reset()
        w0 = time.perf_counter()
        ens.tick(NWATER, NWIND, n=ticks)
        ens.sync()
        wall = time.perf_counter() - w0
        t = ens.timing()
        cs = [m.counters() for m in mem]
    steps = sum(c["steps_water_top"] for c in cs) - s0
    dev_ms = _tick_ms(t) / ticks
    return {"members": b, "ms_per_tick": round(dev_ms, 3), "wall_ms_per_tick": round(1e3 * wall / ticks, 3),
            "phase_ms_per_tick": {k[3:]: round(t[k] / ticks, 3) for k in PHASES},
            "kernel_ms_per_tick": {k: round(t["ms_kernel_" + k] / ticks, 3) for k in ("water", "wind", "classify", "mapfreq")},
            "launches_per_tick": {k: t["launches_" + k] / ticks for k in ("kernel_water", "kernel_wind", "kernel_classify", "kernel_mapfreq")},
            "water_steps_top": steps, "water_steps_per_s": round(steps / (dev_ms * ticks / 1e3), 1),
            "pool_overflow": sum(c["pool_overflow"] for c in cs), "s_to_add_members": round(t_add, 2)}


def run_standalone(cfg, warmup: int, ticks: int) -> dict:
    m = Layermap(cfg, SIZE, SIZE, seed=0, pool=8 * SIZE * SIZE, engine=capi.ENGINE_SERIAL)
    for _ in range(warmup):
        m._chk(m.L.smx_tick(m.h, NWATER, NWIND, 1, 1))
    m.sync()
    s0 = m.counters()["steps_water_top"]
    m.timing_reset()
    w0 = time.perf_counter()
    for _ in range(ticks):
        m._chk(m.L.smx_tick(m.h, NWATER, NWIND, 1, 1))
    m.sync()
    wall = time.perf_counter() - w0
    t = m.timing()
    steps = m.counters()["steps_water_top"] - s0
    m.close()
    dev_ms = _tick_ms(t) / ticks
    return {"ms_per_tick": round(dev_ms, 3), "wall_ms_per_tick": round(1e3 * wall / ticks, 3),
            "phase_ms_per_tick": {k[3:]: round(t[k] / ticks, 3) for k in PHASES}, "water_steps_top": steps}


def run_reference(warmup: int, ticks: int) -> dict:
    """soil_ref_lean for warmup and for warmup + ticks ticks (two processes on two cores): the difference of the phase times is the
    reference's own time for the timed ticks of one member."""
    exe = os.path.join(ROOT, "oracle", "_ref", "soil_ref_lean")
    if not os.path.exists(exe):
        return {"skipped": "oracle/_ref/soil_ref_lean is not built (oracle/Makefile needs the reference tree)"}
    procs = []
    with tempfile.TemporaryDirectory() as td:
        for k, n in enumerate((warmup, warmup + ticks)):
            cmd = [exe, "--soil", os.path.join(ROOT, "soilmachine_amd", "soils", SOIL), "--seed", "0", "--size", str(SIZE), "--ticks", str(n),
                   "--nwater", str(NWATER), "--nwind", str(NWIND), "--wind", "1", "--pool", str(8 * SIZE * SIZE),
                   "--heights-out", os.path.join(td, f"h{k}.bin")]
            procs.append(subprocess.Popen(["taskset", "-c", str(k + 1)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True))
        outs = [p.communicate()[0] for p in procs]
    js = []
    for out in outs:
        j = next((json.loads(line[5:]) for line in out.splitlines() if line.startswith("JSON ")), None)
        if j is None:
            return {"skipped": "soil_ref_lean printed no JSON line"}
        js.append(j)
    tot = [sum(j[k] for k in ("t_water", "t_grid", "t_wind", "t_freq")) for j in js]
    return {"ms_per_tick": round(1e3 * (tot[1] - tot[0]) / ticks, 3), "water_steps_top": js[1]["steps_water_top"] - js[0]["steps_water_top"],
            "binary": "oracle/_ref/soil_ref_lean (the reference's own headers, g++ -O2, one process, one pinned core)"}


# ---------------------------------------------------------------- --observe
OBSERVE_TICKS = 25
TICK_SAMPLES = 5         # ticks 21-25 are timed one by one; their median is the tick the calls are compared with
STREAM_TBS = 5.4          # what the project's own streaming kernels reach (k_map_frequency 5.5, k_lbm_step 5.3 TB/s)
PLANE_BYTES = {"height": 32, "water": 32, "wfreq": 4, "windfreq": 4}   # algorithmic bytes per member and cell and pass


def _median_ms(fn, calls: int, warm: int = 2):
    import statistics
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def _bits(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}") if a.dtype.kind == "f" else a


def run_observe(cfg, b: int, calls: int) -> dict:
    import ctypes as C
    import numpy as np
    pool = 8 * SIZE * SIZE
    cells = SIZE * SIZE
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, SIZE, SIZE, seed=s, pool=pool) for s in range(b)]
        ens.tick(NWATER, NWIND, n=OBSERVE_TICKS - TICK_SAMPLES)
        ens.sync()
        samples = []
        for _ in range(TICK_SAMPLES):                            # the last ticks before the observed state, each timed like the calls below
            t0 = time.perf_counter()
            ens.tick(NWATER, NWIND)
            ens.sync()
            samples.append(1e3 * (time.perf_counter() - t0))
        tick_ms = sorted(samples)[len(samples) // 2]

        # -- figures: one call against B x (smx_digest + getters)
        def per_member():
            out = []
            for m in mem:
                d = m.digest()                                    # smx_digest + the counters (rand_calls)
                ns = C.c_uint64()
                m._chk(m.L.smx_num_sections(m.h, C.byref(ns)))
                ring, idx, rc = (C.c_uint32 * 31)(), C.c_uint32(), C.c_uint64()
                m._chk(m.L.smx_get_rand_state(m.h, ring, C.byref(idx), C.byref(rc)))
                assert int(rc.value) == d["rand_calls"]
                out.append((float(d["sumh"]).hex(), d["nsec"], d["typehash"], d["rand_calls"], int(ns.value)))
            return out

        one = [(float(f["sumh"]).hex(), f["nsec"], f["typehash"], f["rand_calls"], f["live_sections"]) for f in ens.figures()]
        if one != per_member():
            raise SystemExit(f"B={b}: smx_ensemble_figures and the per-member path DISAGREE")
        # ... and the fields smx_digest does not give (water, extremes, empty cells), on the first and the last member, against numpy on exported columns
        figs = ens.figures()
        for i in sorted({0, b - 1}):
            sn = mem[i].snapshot()
            end = np.cumsum(sn.count.astype(np.int64)); nzc = sn.count > 0
            top = end[nzc] - 1
            air = sn.type[top] == 0
            wv = 0.0
            for v in sn.size[top][air]:
                wv += float(v)
            hh = sn.heights()
            want = (int(air.sum()), wv.hex(), float(hh.min()).hex(), float(hh.max()).hex(), int((~nzc).sum()))
            got = (figs[i]["wet_cells"], float(figs[i]["water_volume"]).hex(), float(figs[i]["hmin"]).hex(), float(figs[i]["hmax"]).hex(), figs[i]["empty_cells"])
            if got != want:
                raise SystemExit(f"B={b}: smx_ensemble_figures and numpy on member {i}'s exported columns DISAGREE: {got} vs {want}")
        row = {"members": b, "tick_wall_ms": round(tick_ms, 3), "tick_wall_ms_samples": [round(x, 3) for x in samples], "calls": calls}
        row["figures_ms"], row["figures_ms_min"], row["figures_ms_max"] = _median_ms(ens.figures, calls)
        row["per_member_digest_ms"], row["per_member_digest_ms_min"], row["per_member_digest_ms_max"] = _median_ms(per_member, calls)
        row["figures_speedup"] = round(row["per_member_digest_ms"] / row["figures_ms"], 2)
        row["figures_share_of_tick"] = round(row["figures_ms"] / tick_ms, 5)
        row["per_member_digest_share_of_tick"] = round(row["per_member_digest_ms"] / tick_ms, 5)

        # -- plane statistics: one call against B x smx_read_heights + the numpy member loop
        def heights_loop():
            hs = [m.heights() for m in mem]
            acc = np.zeros(cells); lo = hs[0].copy(); hi = hs[0].copy(); nz = np.zeros(cells, np.uint32)
            for i, v in enumerate(hs):
                acc += v
                if i:
                    lo = np.where(v < lo, v, lo); hi = np.where(v > hi, v, hi)
                nz += (v != 0.0).astype(np.uint32)
            mean = acc / float(len(hs))
            a2 = np.zeros(cells)
            for v in hs:
                d = v - mean
                a2 += d * d
            return {"mean": mean, "var": a2 / float(len(hs)), "vmin": lo, "vmax": hi, "nonzero": nz}

        got, want = ens.plane_stats("height"), heights_loop()
        for k in want:
            if not np.array_equal(_bits(got[k]), _bits(want[k])):
                raise SystemExit(f"B={b}: smx_ensemble_plane_stats(height) and the per-member numpy loop DISAGREE in {k}")
        row["per_member_heights_ms"], _, _ = _median_ms(heights_loop, calls)
        planes = {}
        for plane in ("height", "water", "wfreq", "windfreq"):
            for var in (True, False):
                ms, lo, hi = _median_ms(lambda: ens.plane_stats(plane, var=var), calls)
                gb = b * cells * PLANE_BYTES[plane] * (2 if var else 1) / 1e9
                planes[plane + ("_var" if var else "")] = {"ms": ms, "ms_min": lo, "ms_max": hi, "algorithmic_gb": round(gb, 6),
                                                           "gb_per_s": round(gb / (ms / 1e3), 2), "share_of_stream_rate": round(gb / (ms / 1e3) / (1e3 * STREAM_TBS), 5),
                                                           "share_of_tick": round(ms / tick_ms, 5)}
        row["plane_stats"] = planes
        row["heights_speedup"] = round(row["per_member_heights_ms"] / planes["height_var"]["ms"], 2)
    return row


def main_observe(a):
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    rec = {"workload": {"soil": SOIL, "size": SIZE, "nwater": NWATER, "nwind": NWIND, "seeds": "0..B-1", "pool_sections_per_cell": 8,
                        "state": f"after tick {OBSERVE_TICKS}", "tick": f"median wall clock of the last {TICK_SAMPLES} ticks, each followed by a sync", "calls": a.calls, "warmup_calls": 2,
                        "clock": "wall clock around blocking calls; median (min, max) of `calls`",
                        "stream_rate_tb_s": STREAM_TBS},
           "observe": []}
    for b in (int(x) for x in a.batches.split(",") if x):
        r = run_observe(cfg, b, a.calls)
        rec["observe"].append(r)
        print(f"[observe] B={b:5d}  figures {r['figures_ms']:9.3f} ms  per-member {r['per_member_digest_ms']:10.3f} ms  x{r['figures_speedup']:.1f}   "
              f"height stats {r['plane_stats']['height_var']['ms']:8.3f} ms  per-member {r['per_member_heights_ms']:9.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    if not a.no_record:
        os.makedirs(a.out, exist_ok=True)
        stem = os.path.join(a.out, f"r09_ensemble_{a.tag if a.tag != 'bench' else 'observe'}")
        with open(stem + ".json", "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        write_observe_md(rec, stem + ".md")


MD_MARK = "## Measurement"


def write_observe_md(rec: dict, path: str):
    """The table of the record as markdown: everything from the line '## Measurement' on is rewritten, what stands before it (the
    kernel resources, written from the compiler's remarks) is kept."""
    head = ""
    if os.path.exists(path):
        head = open(path).read().split(MD_MARK)[0]
    w = rec["workload"]
    out = [MD_MARK + f" (`tools/ensemble_bench.py --observe`, {os.path.basename(path)[:-3]}.json)", "",
           f"{w['size']}² `{w['soil']}`, {w['nwater']} + {w['nwind']} particles, seeds {w['seeds']}, {w['pool_sections_per_cell']} pool sections per cell, state {w['state']}. "
           f"Times: {w['clock']} ({w['calls']} calls after {w['warmup_calls']} warm-up calls); tick = {w['tick']}. Both paths agreed bit for bit before a time was taken (sumh, nsec, typehash, rand_calls, live_sections on every member; the water fields, extremes and empty cells on the first and the last member against numpy on exported columns; all five outputs of the height statistics).", "",
           "| B | tick ms | `figures()` ms | B × `smx_digest` + getters ms | speed-up | `figures()` / tick | per-member / tick | height stats (var) ms | B × `smx_read_heights` + numpy ms | speed-up |",
           "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in rec["observe"]:
        out.append(f"| {r['members']} | {r['tick_wall_ms']:.1f} | {r['figures_ms']:.3f} | {r['per_member_digest_ms']:.2f} | {r['figures_speedup']:.1f} × | "
                   f"{100 * r['figures_share_of_tick']:.2f} % | {100 * r['per_member_digest_share_of_tick']:.1f} % | {r['plane_stats']['height_var']['ms']:.3f} | "
                   f"{r['per_member_heights_ms']:.2f} | {r['heights_speedup']:.1f} × |")
    out += ["", f"`plane_stats`: ms, algorithmic GB/s (members × cells × 32 B per pass for height / water, 4 B for the frequency planes; two passes with var) "
                f"and the share of the {w['stream_rate_tb_s']} TB/s the project's streaming kernels reach:", "",
            "| B | " + " | ".join(k.replace("_var", " +var") for k in rec["observe"][0]["plane_stats"]) + " |",
            "|---:|" + "---:|" * len(rec["observe"][0]["plane_stats"])]
    for r in rec["observe"]:
        out.append(f"| {r['members']} | " + " | ".join(f"{v['ms']:.3f} ms, {v['gb_per_s']:.0f} GB/s, {100 * v['share_of_stream_rate']:.1f} %" for v in r["plane_stats"].values()) + " |")
    with open(path, "w") as f:
        f.write(head + "\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--observe", action="store_true", help="time smx_ensemble_figures / _plane_stats against the per-member path")
    ap.add_argument("--calls", type=int, default=10, help="--observe: timed calls per figure (after 2 warm-up calls)")
    ap.add_argument("--batches", default="1,8,64,256,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--no-record", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of the record (default: profiles/)")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--no-standalone", action="store_true")
    a = ap.parse_args()
    if a.observe:
        return main_observe(a)
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    rec = {"workload": {"soil": SOIL, "size": SIZE, "nwater": NWATER, "nwind": NWIND, "seeds": "0..B-1", "pool_sections_per_cell": 8,
                        "warmup": a.warmup, "ticks": a.ticks}}
    if not a.no_standalone:
        rec["standalone_serial"] = run_standalone(cfg, a.warmup, a.ticks)
    rows = []
    for b in (int(x) for x in a.batches.split(",") if x):
        r = run_ensemble(cfg, b, a.warmup, a.ticks)
        rows.append(r)
        print(f"[ensemble] B={b:5d}  {r['ms_per_tick']:9.2f} ms/tick  {r['water_steps_per_s'] / 1e6:8.3f} M water steps/s", file=sys.stderr, flush=True)
    base = next((r for r in rows if r["members"] == 1), None)
    for r in rows:
        if base:
            r["slowdown_per_member_vs_b1"] = round(r["ms_per_tick"] / base["ms_per_tick"], 3)
            r["throughput_vs_b1"] = round(r["members"] * base["ms_per_tick"] / r["ms_per_tick"], 2)
    rec["ensembles"] = rows
    if not a.no_ref:
        ref = run_reference(a.warmup, a.ticks)
        rec["reference_one_core"] = ref
        if "ms_per_tick" in ref:
            for r in rows:
                r["host_cores_equivalent"] = round(r["members"] * ref["ms_per_tick"] / r["ms_per_tick"], 2)
    floors = {}
    sa = rec.get("standalone_serial")
    if base and sa:
        floors["b1_within_10pct_of_standalone"] = base["ms_per_tick"] <= 1.10 * sa["ms_per_tick"]
        floors["b1_over_standalone"] = round(base["ms_per_tick"] / sa["ms_per_tick"], 3)
    r256 = next((r for r in rows if r["members"] == 256), None)
    if base and r256:
        floors["b256_at_most_8x_b1"] = r256["ms_per_tick"] <= 8.0 * base["ms_per_tick"]
        floors["b256_over_b1"] = round(r256["ms_per_tick"] / base["ms_per_tick"], 3)
    rec["floors"] = floors
    line = json.dumps(rec)
    print(line, flush=True)
    if not a.no_record:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"r07_ensemble_{a.tag}.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
