#!/usr/bin/env python3
"""Ensembles of exact maps (smx_ensemble_*): the tick of B members against one standalone SERIAL context and the reference's
one-core loop. Workload: default.soil at 256^2, 250 water + 250 wind particles per tick, seeds 0..B-1, pools of 8 sections per
cell; 5 warm-up ticks, 20 timed. Prints one JSON line and writes profiles/r07_ensemble_<tag>.json.

usage: ensemble_bench.py [--batches 1,8,64,256,1024] [--warmup 5] [--ticks 20] [--tag bench] [--out profiles] [--no-record] [--no-ref]
       ensemble_bench.py --observe [--batches 1,8,64,256,1024] [--calls 10] [--tag observe]     (writes profiles/r09_ensemble_<tag>.json)
       ensemble_bench.py --fork [--batches 8,64,256,1024] [--calls 5] [--tag fork] [--no-big]    (writes profiles/r10_ensemble_<tag>.json / .md)

--fork: a spun-up map branched into B members (smx_ensemble_fork) against the path without it: one snapshot() of the source, then per
member Ensemble.add(initialize off) + load + smx_set_rand_state. Source: the workload below after tick 25. Both paths run in this
process, alternating, `calls` times each; both must give bit-identical members before a time is taken. Plus one line for a 4096^2
rockgravelpebblessand source after 5 relaxed ticks, forked into 4 members. SMX_FORK_PROFILE_ONLY=B runs just the fork of B members,
SMX_FORK_PROFILE_ONLY=1024x8 one fork of a 1024^2 rockgravelpebblessand source (deep columns) into 8 (each for a kernel trace); --scatter-stats FILE folds such a trace's k_fork_scatter time into the record.

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


# ---------------------------------------------------------------- --fork
FORK_TICKS = 25
BIG = {"soil": "rockgravelpebblessand.soil", "size": 4096, "nwater": 64000, "nwind": 16000, "ticks": 5, "members": 4}


def _rand_state(m):
    import ctypes as C
    ring, idx, calls = (C.c_uint32 * 31)(), C.c_uint32(), C.c_uint64()
    m._chk(m.L.smx_get_rand_state(m.h, ring, C.byref(idx), C.byref(calls)))
    return ring, int(idx.value), int(calls.value)


def fork_bytes(snap, cap: int, members: int) -> dict:
    """The bytes the algorithm must move, from the section counts: the count pass reads every record once; per member the scatter
    reads every record, the two count words and the flag byte per cell, and writes the records, the flag bytes and the free list; the
    plane copy reads and writes three f32 planes."""
    n, total = snap.ncells, snap.nsec
    used = total - int((snap.count > 0).sum())
    rec = 32 * (n + used)
    count = rec + n + 9 * n
    scatter = (rec + 9 * n) + (rec + n + 4 * (cap - used))
    planes = 2 * 12 * n
    return {"cells": n, "sections": total, "buried": used, "count_pass": count, "scatter_per_member": scatter, "planes_per_member": planes,
            "total": count + members * (scatter + planes)}


def _fork_once(src, b, pool):
    ens = Ensemble(0)
    t0 = time.perf_counter()
    mem = ens.fork(src, b, pool=pool)
    return ens, mem, 1e3 * (time.perf_counter() - t0)


def _parent_once(src, b, pool):
    ens = Ensemble(0)
    t0 = time.perf_counter()
    snap = src.snapshot()
    ring, idx, calls = _rand_state(src)
    mem = []
    for _ in range(b):
        m = ens.add(src.cfg, src.dimx, src.dimy, seed=0, pool=pool, initialize=False)
        m.load(snap)
        m._chk(m.L.smx_set_rand_state(m.h, ring, idx, calls))
        mem.append(m)
    return ens, mem, 1e3 * (time.perf_counter() - t0)


def _check_identical(b, ea, ma, eb, mb):
    from soilmachine_amd.snapshot import compare
    key = lambda f: (float(f["sumh"]).hex(), f["nsec"], f["typehash"], f["rand_calls"], f["live_sections"], f["wet_cells"], float(f["water_volume"]).hex())
    fa, fb = [key(f) for f in ea.figures()], [key(f) for f in eb.figures()]
    if fa != fb or len(set(fa)) != 1:
        raise SystemExit(f"B={b}: the forked members and the loaded members DISAGREE (figures)")
    for i in sorted({0, b - 1}):
        bad = compare(ma[i].snapshot(), mb[i].snapshot())
        ra, rb = _rand_state(ma[i]), _rand_state(mb[i])
        if bad or (tuple(ra[0]), ra[1:]) != (tuple(rb[0]), rb[1:]) or ma[i].counters() != mb[i].counters():
            raise SystemExit(f"B={b}: forked member {i} and loaded member {i} DISAGREE: {bad}")


def run_fork(src, snap, b: int, calls: int, pool: int) -> dict:
    import statistics
    ea, ma, _ = _fork_once(src, b, pool)
    eb, mb, _ = _parent_once(src, b, pool)
    _check_identical(b, ea, ma, eb, mb)
    ea.close(); eb.close()
    tf, tp = [], []
    for _ in range(calls):                                     # alternating: fork, parent path, fork, ...
        e, _, ms = _fork_once(src, b, pool); tf.append(ms); e.close()
        e, _, ms = _parent_once(src, b, pool); tp.append(ms); e.close()
    by = fork_bytes(snap, pool, b)
    f_ms, p_ms = statistics.median(tf), statistics.median(tp)
    return {"members": b, "calls": calls, "fork_ms": round(f_ms, 3), "fork_ms_min": round(min(tf), 3), "fork_ms_max": round(max(tf), 3),
            "parent_path_ms": round(p_ms, 3), "parent_path_ms_min": round(min(tp), 3), "parent_path_ms_max": round(max(tp), 3),
            "speedup": round(p_ms / f_ms, 2), "algorithmic_bytes": by, "fork_gb_per_s": round(by["total"] / 1e9 / (f_ms / 1e3), 2)}


def run_fork_big(calls: int) -> dict:
    from soilmachine_amd.snapshot import compare
    import statistics
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", BIG["soil"]))
    src = Layermap(cfg, BIG["size"], BIG["size"], seed=0, engine=capi.ENGINE_RELAXED)
    for _ in range(BIG["ticks"]):
        src._chk(src.L.smx_tick(src.h, BIG["nwater"], BIG["nwind"], 1, 1))
    src.sync()
    snap = src.snapshot()
    ts = []
    for k in range(calls + 1):
        e, mem, ms = _fork_once(src, BIG["members"], None)
        if k == 0:                                              # (warm-up call: checked against the source's exported state)
            figs = e.figures()
            d = snap.digest() if snap.ncells <= 1 << 16 else None
            if len({(f["nsec"], f["typehash"], float(f["sumh"]).hex()) for f in figs}) != 1 or figs[0]["nsec"] != snap.nsec or (d and d["typehash"] != figs[0]["typehash"]):
                raise SystemExit("4096^2: the forked members differ from the source")
            bad = compare(mem[-1].snapshot(), snap)
            if bad:
                raise SystemExit(f"4096^2: the last forked member differs from the source: {bad}")
        else:
            ts.append(ms)
        e.close()
    by = fork_bytes(snap, src.pool, BIG["members"])
    src.close()
    ms = statistics.median(ts)
    return {**BIG, "engine": "relaxed", "pool_sections": src.pool, "calls": calls, "fork_ms": round(ms, 3), "fork_ms_min": round(min(ts), 3), "fork_ms_max": round(max(ts), 3),
            "parent_path_ms": "not measured", "algorithmic_bytes": by, "fork_gb_per_s": round(by["total"] / 1e9 / (ms / 1e3), 2)}


def scatter_stats(path: str) -> dict:
    """k_fork_scatter / k_fork_count / k_fork_planes out of a rocprofv3 --kernel-trace --stats CSV (*_kernel_stats.csv)."""
    import csv
    import glob
    out = {}
    if os.path.isdir(path):                                     # (rocprofv3 -d DIR: the file sits in a sub-directory named after the host)
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            return out
        path = found[0]
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in ("k_fork_scatter", "k_fork_count", "k_fork_planes"):
                if k in name:
                    out[k] = {"calls": int(row["Calls"]), "total_ns": int(float(row["TotalDurationNs"])), "average_ns": float(row["AverageNs"])}
    return out


def profile_deep(size: int, members: int):
    """One fork of a size^2 rockgravelpebblessand source (deep columns) after 3 relaxed ticks with area-scaled particle counts: the run
    a kernel trace is taken of, to see what the deepest columns cost a lane-per-cell scatter."""
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", BIG["soil"]))
    k = (size / 256.0) ** 2
    src = Layermap(cfg, size, size, seed=0, pool=32 * size * size, engine=capi.ENGINE_RELAXED)
    for _ in range(3):
        src._chk(src.L.smx_tick(src.h, int(250 * k), int(62.5 * k), 1, 1))
    src.sync()
    snap = src.snapshot()
    pool = snap.nsec + 4 * size * size
    e, _, ms = _fork_once(src, members, pool)
    print(json.dumps({"profile_only": f"{size}x{members}", "soil": BIG["soil"], "fork_ms": round(ms, 3), "deepest_column": int(snap.count.max()),
                      "mean_column": round(snap.nsec / snap.ncells, 2), "pool": pool, "algorithmic_bytes": fork_bytes(snap, pool, members)}), flush=True)
    e.close(); src.close()


def main_fork(a):
    only = os.environ.get("SMX_FORK_PROFILE_ONLY")
    if only and "x" in only:
        return profile_deep(*(int(v) for v in only.split("x")))
    cfg = loadsoil(os.path.join(ROOT, "soilmachine_amd", "soils", SOIL))
    pool = 8 * SIZE * SIZE
    src = Layermap(cfg, SIZE, SIZE, seed=0, pool=pool, engine=capi.ENGINE_SERIAL)
    for _ in range(FORK_TICKS):
        src._chk(src.L.smx_tick(src.h, NWATER, NWIND, 1, 1))
    src.sync()
    snap = src.snapshot()
    if only:                                                    # one fork, nothing else: the run a kernel trace is taken of
        e, _, ms = _fork_once(src, int(only), pool)
        print(json.dumps({"profile_only": int(only), "fork_ms": round(ms, 3), "algorithmic_bytes": fork_bytes(snap, pool, int(only))}), flush=True)
        e.close(); src.close()
        return
    rec = {"workload": {"soil": SOIL, "size": SIZE, "nwater": NWATER, "nwind": NWIND, "seed": 0, "pool_sections_per_cell": 8, "state": f"after tick {FORK_TICKS}",
                        "sections": snap.nsec, "deepest_column": int(snap.count.max()), "calls": a.calls,
                        "clock": "wall clock around the blocking calls (member creation included, destruction not), the two paths alternating; median (min, max)",
                        "parent_path": "one snapshot() of the source, then per member Ensemble.add(initialize off) + load + smx_set_rand_state",
                        "checked": "before a time is taken: figures() of all members of both paths equal; snapshot, generator and counters of the first and the last member equal",
                        "stream_rate_tb_s": STREAM_TBS},
           "fork": []}
    for b in (int(x) for x in a.batches.split(",") if x):
        r = run_fork(src, snap, b, a.calls, pool)
        rec["fork"].append(r)
        print(f"[fork] B={b:5d}  fork {r['fork_ms']:10.3f} ms  parent path {r['parent_path_ms']:11.3f} ms  x{r['speedup']:.1f}", file=sys.stderr, flush=True)
    src.close()
    if not a.no_big:
        rec["fork_4096"] = run_fork_big(max(3, a.calls))
        print(f"[fork] 4096^2 x {BIG['members']}: {rec['fork_4096']['fork_ms']:.1f} ms", file=sys.stderr, flush=True)
    rec["k_fork_scatter"] = "not measured"
    if a.scatter_stats:
        st = scatter_stats(a.scatter_stats)
        b = a.scatter_members
        by = fork_bytes(snap, pool, b)
        if "k_fork_scatter" in st:
            sec = st["k_fork_scatter"]["total_ns"] / 1e9
            rec["k_fork_scatter"] = {"members": b, "kernels": st, "scatter_bytes": b * by["scatter_per_member"], "gb_per_s": round(b * by["scatter_per_member"] / 1e9 / sec, 1),
                                     "share_of_stream_rate": round(b * by["scatter_per_member"] / 1e9 / sec / (1e3 * STREAM_TBS), 4),
                                     "source": "a separate rocprofv3 --kernel-trace --stats run of SMX_FORK_PROFILE_ONLY=" + str(b)}
    print(json.dumps(rec), flush=True)
    if not a.no_record:
        os.makedirs(a.out, exist_ok=True)
        stem = os.path.join(a.out, f"r10_ensemble_{a.tag if a.tag != 'bench' else 'fork'}")
        with open(stem + ".json", "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        write_fork_md(rec, stem + ".md")


def write_fork_md(rec: dict, path: str):
    head = ""
    if os.path.exists(path):
        head = open(path).read().split(MD_MARK)[0]
    w = rec["workload"]
    out = [MD_MARK + f" (`tools/ensemble_bench.py --fork`, {os.path.basename(path)[:-3]}.json)", "",
           f"Source: {w['size']}² `{w['soil']}`, {w['nwater']} + {w['nwind']} particles, seed {w['seed']}, {w['pool_sections_per_cell']} pool sections per cell, {w['state']} "
           f"({w['sections']} sections, deepest column {w['deepest_column']}). Parent path: {w['parent_path']}. Times: {w['clock']} of {w['calls']} calls. Checked {w['checked']}.", "",
           "| B | `fork` ms (min, max) | parent path ms (min, max) | speed-up | bytes the fork must move | fork GB/s (whole call) |",
           "|---:|---:|---:|---:|---:|---:|"]
    for r in rec["fork"]:
        out.append(f"| {r['members']} | {r['fork_ms']:.2f} ({r['fork_ms_min']:.2f}, {r['fork_ms_max']:.2f}) | {r['parent_path_ms']:.1f} ({r['parent_path_ms_min']:.1f}, {r['parent_path_ms_max']:.1f}) | "
                   f"{r['speedup']:.1f} × | {r['algorithmic_bytes']['total'] / 1e6:.1f} MB | {r['fork_gb_per_s']:.1f} |")
    g = rec.get("fork_4096")
    if g:
        out += ["", f"{g['size']}² `{g['soil']}` after {g['ticks']} relaxed ticks ({g['nwater']} + {g['nwind']} particles, pool {g['pool_sections']} sections, {g['algorithmic_bytes']['sections']} live), "
                    f"forked into {g['members']} members with the source's pool size: {g['fork_ms']:.1f} ms ({g['fork_ms_min']:.1f}, {g['fork_ms_max']:.1f}) for {g['algorithmic_bytes']['total'] / 1e9:.2f} GB "
                    f"= {g['fork_gb_per_s']:.0f} GB/s over the whole call; parent path: {g['parent_path_ms']}."]
    k = rec.get("k_fork_scatter")
    if isinstance(k, dict):
        ks = k["kernels"]
        out += ["", f"`k_fork_scatter` alone ({k['source']}): {ks['k_fork_scatter']['total_ns'] / 1e3:.1f} µs for {k['scatter_bytes'] / 1e6:.1f} MB = {k['gb_per_s']:.0f} GB/s, "
                    f"{100 * k['share_of_stream_rate']:.1f} % of the {w['stream_rate_tb_s']} TB/s measured for `k_map_frequency`"
                    + "".join(f"; `{n}` {v['total_ns'] / 1e3:.1f} µs" for n, v in ks.items() if n != "k_fork_scatter") + "."]
    else:
        out += ["", "`k_fork_scatter`'s own rate: not measured."]
    with open(path, "w") as f:
        f.write(head + "\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fork", action="store_true", help="time smx_ensemble_fork against snapshot + per-member add / load")
    ap.add_argument("--no-big", action="store_true", help="--fork: leave the 4096^2 line out")
    ap.add_argument("--scatter-stats", default=None, metavar="CSV", help="--fork: a rocprofv3 kernel-stats CSV of an SMX_FORK_PROFILE_ONLY run")
    ap.add_argument("--scatter-members", type=int, default=256, help="--fork: the B of that run")
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
    if a.fork:
        if a.batches == "1,8,64,256,1024":
            a.batches = "8,64,256,1024"
        if a.calls == 10:
            a.calls = 5
        return main_fork(a)
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
