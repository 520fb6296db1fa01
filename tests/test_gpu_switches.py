"""Every results-neutral run-time switch on the device (README.md "Run-time switches", the table behind smx_switches).

The library reads its SMX_* switches once per process, so every setting of the matrix below runs in a child process of its own
(tests/switch_child.py: all scenarios of one engine, one JSON document), one child at a time. The parent computes what the
scenarios must give on the CPU -- golden snapshots of the reference and the oracle in the reference's order for the exact engines,
the oracle's restated schedules for the batched and the relaxed engine, the same headers on host threads for the relaxed engine with
relaxed wind, the restated shaders for the LBM -- once per scenario, and asserts EQUALITY: the state after every tick (every array,
as common.snapshot_hashes) and the counters at the end. The switches are the only way to reach at 64^2 what the benchmark runs at
4096^2: wavefronts that take many tickets of a dataflow kernel, 64 particles per wavefront with a partly filled last one, the
256-register epoch kernel, the per-phase launches of a relaxed epoch.

Every test also reads the child's switch table: the switches it set were read with the intended, non-default values, every other
switch is at its default -- a misspelt name fails there instead of passing vacuously. test_every_neutral_switch_has_a_setting holds
the matrix complete: a `neutral` switch that no setting moves off its default fails it.

Trouble ends it: a child that runs into its time limit, dies of a signal or reports an illegal memory access fails its test and
sets FIRST_FAULT; every later test of the module then fails at once, naming it, and starts no child. Nothing is retried.
Time limits: profiles/r10_switch_children.md has each child's measured run time.
"""
from __future__ import annotations

import functools
import json
import os
import subprocess
import sys
import time

import pytest

import switch_child as sc
from common import ROOT, golden_snapshot, load_cfg, snapshot_hashes, digests, case_dims, SNAP_CASES

CHILD = os.path.join(ROOT, "tests", "switch_child.py")
# seconds a child may take. The slowest child measured on an MI355X took 13.9 s (speculative, SMX_SPEC_MODE=0 SMX_SPEC_MODE_WIND=0), a
# relaxed one 4-6 s, a batched one 3-4 s, an LBM one 0.4 s (profiles/r10_switch_children.md); the machine is shared, hence the margin
CHILD_TIMEOUT = 120
FIRST_FAULT = None                                     # the first child that hung, died of a signal or faulted the device

EXACT_KEYS = ["steps_water_top", "steps_water_all", "steps_wind", "nested_particles", "floods", "cascade_calls", "cascade_transfers",
              "wcascade_calls", "rand_calls"]
BATCH_KEYS = EXACT_KEYS + ["pool_free"]

# ---- the matrix: (engine, setting). Every value lies inside the clamps of csrc/soilmx.hip (noted where there is one). ----
# The two settings with few wavefronts in a dataflow kernel (SMX_RELAX_CASC_FLOW=2, SMX_GRID_FLOW_WAVES=3): forward progress is the
# argument above spin_wait_while and holds for every count >= 1. k_relax_cascade_flow and k_grid_tiles_flow hand out tickets from one
# atomic cursor in (colour, cell) order; ticket i waits only for cells / tiles of EARLIER colours, i.e. for tickets j < i; only a
# wavefront that is running takes a ticket. So the lowest unfinished ticket is always held by a running wavefront whose dependencies
# are all finished: it completes, whatever the number of wavefronts and whether or not they are resident together. With 2 and 3
# wavefronts every wavefront loops over many tickets (a 64^2 map lists tens to hundreds of cells and up to 256 tiles), as at the
# headline size. (SMX_RELAX_CASC_FLOW=0 is not a dataflow launch; 1 would serialise it and wait for nothing.)
# Under the default tail rule (one workgroup runs whole epochs once <= 256 particles run) the scenarios' water phases never reach the
# per-phase launches: the settings marked (*) add SMX_RELAX_TAIL=0 to the one above them so that the water epochs run through them too.
MATRIX = [
    ("speculative", {"SMX_COOP": "0"}),
    ("speculative", {"SMX_COOP": "0", "SMX_SPEC_LANES": "8"}),          # (100 / 250 / 60 / 50 / 40 particles: no multiple of 8 but 40)
    ("speculative", {"SMX_COOP": "0", "SMX_SPEC_LANES": "64"}),         # (clamp 1..64)
    ("speculative", {"SMX_SPEC_MODE": "0", "SMX_SPEC_MODE_WIND": "0"}),
    ("speculative", {"SMX_SPEC_MODE": "1", "SMX_SPEC_MODE_WIND": "3"}),
    ("speculative", {"SMX_SPEC_MODE": "2"}),
    ("speculative", {"SMX_WIND_SCOUT": "0"}),
    ("speculative", {"SMX_SPEC_SUB": "64", "SMX_SPEC_MAXNEST": "128"}),  # (the clamps' lower ends: >= 64, 128..60000)
    ("serial", {"SMX_CLASSIFY_SCALAR": "1"}),
    ("batched", {"SMX_BATCH_OCC2_ABOVE": "0"}),
    ("batched", {"SMX_BATCH_WAVES": "0"}),
    ("batched", {"SMX_BATCH_WAVES": "3"}),
    ("batched", {"SMX_BATCH_WAVES": "100000"}),
    ("relaxed", {"SMX_BATCH_WAVES": "0"}),
    ("relaxed", {"SMX_RELAX_CASC_FLOW": "0"}),
    ("relaxed", {"SMX_RELAX_CASC_FLOW": "0", "SMX_RELAX_TAIL": "0"}),                                   # (*)
    ("relaxed", {"SMX_RELAX_CASC_FLOW": "0", "SMX_RELAX_CASC_BLOCKS": "1"}),
    ("relaxed", {"SMX_RELAX_CASC_FLOW": "0", "SMX_RELAX_CASC_BLOCKS": "1", "SMX_RELAX_TAIL": "0"}),      # (*)
    ("relaxed", {"SMX_RELAX_CASC_FLOW": "2", "SMX_GRID_FLOW_WAVES": "3"}),
    ("relaxed", {"SMX_RELAX_CASC_FLOW": "2", "SMX_GRID_FLOW_WAVES": "3", "SMX_RELAX_TAIL": "0"}),        # (*)
    ("relaxed", {"SMX_RELAX_FLOOD_BLOCKS": "1"}),
    ("relaxed", {"SMX_RELAX_FLOOD_BLOCKS": "1", "SMX_RELAX_TAIL": "0", "SMX_BATCH_WAVES": "0"}),         # (*) (floods: max(1, ceil(slots / 64)) wavefronts, up to 64 floods each)
    ("relaxed", {"SMX_RELAX_TAIL": "0"}),
    ("relaxed", {"SMX_RELAX_TAIL": "0", "SMX_RELAX_CHUNK_KIDS": "3"}),
    ("relaxed", {"SMX_RELAX_TAIL_AT": "100000"}),
    ("relaxed", {"SMX_RELAX_MEGA": "1", "SMX_RELAX_MEGA_WAVES": "5", "SMX_RELAX_MEGA_CHUNK": "5", "SMX_RELAX_MEGA_FLAGS": "1"}),
    ("relaxed", {"SMX_RELAX_MEGA": "1", "SMX_RELAX_MEGA_WAVES": "5", "SMX_RELAX_MEGA_CHUNK": "5", "SMX_RELAX_MEGA_FLAGS": "1",
                 "SMX_RELAX_MEGA_BLOCKS": "7", "SMX_RELAX_TAIL": "0"}),                                   # (*) (7 workgroups = 28 wavefronts, 5 of them in the dense phases)
    ("relaxed", {"SMX_GRID_POLL_NAPS": "0"}),
    ("relaxed", {"SMX_CLASSIFY_SCALAR": "1"}),
    ("lbm", {"SMX_LBM_NT": "1"}),
    ("lbm", {"SMX_LBM_XCD": "1"}),
    ("lbm", {"SMX_LBM_NT": "1", "SMX_LBM_XCD": "1"}),
]


def setting_id(p):
    return p[0] + ":" + ",".join(f"{k[4:]}={v}" for k, v in p[1].items())


# ------------------------------------------------------------------------------------------------ what the scenarios must give (CPU)
@functools.lru_cache(maxsize=None)
def expected(engine: str) -> dict:
    from hostsim_lib import HostSim
    from oracle_lib import LbmOracle, Oracle
    out = {}
    if engine in ("speculative", "serial"):
        # the oracle in the reference's order, every tick; at the ticks with a golden snapshot of the reference itself it must be that snapshot
        dig = digests()
        for name, (soil, case, seed, wind, ticks) in sc.SCENARIOS[engine].items():
            cfg = load_cfg(soil)
            d = dig[case]
            dimx, dimy = case_dims(d, cfg)
            o = Oracle(cfg, dimx, dimy, seed=seed); o.initialize()
            hashes = []
            for _ in range(ticks):
                o.tick(d["nwater"], d["nwind"], True, wind)
                hashes.append(snapshot_hashes(o.snapshot()))
            golden = [t for t in SNAP_CASES[case][3] if 0 < t <= ticks]
            assert ticks in golden
            for t in golden:
                assert hashes[t - 1] == snapshot_hashes(golden_snapshot(case, t)), (case, t)
            c = o.counters()
            assert (c["steps_water_top"], c["steps_wind"]) == (d["steps_water_top"], d["steps_wind"])
            out[name] = {"hashes": hashes, "counters": {k: c[k] for k in EXACT_KEYS}}
    elif engine == "batched":
        for name, (soil, case, t0, nw, nd, wind, ticks, dilate) in sc.BATCHED.items():
            cfg, g = load_cfg(soil), golden_snapshot(case, t0)
            o = Oracle(cfg, g.dimx, g.dimy, seed=0); o.load(g); o.batched_set_dilate(dilate)
            hashes = []
            for _ in range(ticks):
                o.batched_tick(nw, nd, True, wind)
                hashes.append(snapshot_hashes(o.snapshot()))
            c, st = o.counters(), o.batched_stats()
            assert st["guard_violations"] == 0
            out[name] = {"hashes": hashes, "counters": {k: c[k] for k in BATCH_KEYS},
                         "batch_stats": {"epochs": st["epochs"], "generations": st["generations"], "children_lost": 0}}
    elif engine == "relaxed":
        for name, (ref, soil, case, t0, nw, nd, wind, ticks, wmin, wsteps) in sc.RELAXED.items():
            cfg, g = load_cfg(soil), golden_snapshot(case, t0)
            hashes = []
            if ref == "oracle":
                o = Oracle(cfg, g.dimx, g.dimy, seed=0); o.load(g)
                for _ in range(ticks):
                    o.relaxed_tick(nw, nd, True, wind)
                    hashes.append(snapshot_hashes(o.snapshot()))
                assert o.batched_stats()["guard_violations"] == 0
                c = o.counters()
                out[name] = {"hashes": hashes, "counters": {k: c[k] for k in EXACT_KEYS}}
            else:
                h = HostSim(cfg, g.dimx, g.dimy, seed=0); h.load(g, advance_rand=True)
                for t in range(ticks):
                    h.relaxed_tick(nw, nd, True, wind, nthreads=4, shuffle=t + 1, wind_min=wmin, wind_steps=wsteps)
                    hashes.append(snapshot_hashes(h.snapshot()))
                c = h.counters()
                out[name] = {"hashes": hashes, "counters": {k: c[k] for k in BATCH_KEYS}}
    elif engine == "lbm":
        for name, dims in sc.LBM.items():
            o = LbmOracle(*dims)
            out[name] = sc.lbm_run(o, dims, o.read)
    return out


# ------------------------------------------------------------------------------------------------ one child
def run_child(engine: str, setting: dict) -> dict:
    global FIRST_FAULT
    if FIRST_FAULT:
        pytest.fail(f"not started: an earlier child of this module ended in trouble -- {FIRST_FAULT}")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SMX_")}
    env.update(setting)
    what = f"{engine} under {setting}"
    t0 = time.monotonic()
    try:
        r = subprocess.run([sys.executable, CHILD, engine], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        FIRST_FAULT = f"{what}: no end within {CHILD_TIMEOUT} s"
        pytest.fail(FIRST_FAULT)
    print(f"[switch-child] {what}: {time.monotonic() - t0:.1f} s, exit status {r.returncode}")
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr:
        FIRST_FAULT = f"{what}: exit status {r.returncode}; stderr ends: {r.stderr[-600:]!r}"
        pytest.fail(FIRST_FAULT)
    assert r.returncode == 0, (what, r.returncode, r.stdout[-400:], r.stderr[-1200:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("SWITCH-CHILD-JSON ")]
    assert len(lines) == 1, (what, r.stdout[-400:])
    doc = json.loads(lines[0][len("SWITCH-CHILD-JSON "):])
    print("[switch-child]   scenarios:", ", ".join(f"{k} {v['seconds']} s" for k, v in doc["scenarios"].items()))
    return doc


def check_table(table: dict, setting: dict):
    """the switches of the setting were read, with non-default values; every other switch is at its default"""
    for k, v in setting.items():
        assert k in table, f"{k} is no switch of the library"
        assert table[k]["value"] == v and table[k]["value"] != table[k]["default"], (k, table[k])
    off = {k: e for k, e in table.items() if k not in setting and e["value"] != e["default"]}
    assert not off, off


def check_path(engine: str, setting: dict, doc: dict):
    """where timing() or the counters show which path ran"""
    sets = lambda k, v: setting.get(k) == v
    for name, res in doc["scenarios"].items():
        if engine == "lbm":
            assert res["timing"]["steps"] == sc.LBM_STEPS
            continue
        t, c = res["timing"], res["counters"]
        assert c["pool_overflow"] == 0
        if engine in ("speculative", "serial") or sets("SMX_CLASSIFY_SCALAR", "1"):
            assert t["launches_kernel_classify"] > 0, name
        if engine == "speculative":
            assert c["spec_rounds"] > 0, (name, c)
        if engine == "relaxed":
            if sets("SMX_RELAX_TAIL", "0"):
                assert t["launches_kernel_tail"] == 0 and t["epochs_kernel_tail"] == 0, name
                if sets("SMX_RELAX_MEGA", "1"):            # every epoch with a running water particle is the persistent kernel's
                    assert t["launches_kernel_epochs"] > 0 and t["epochs_kernel_epochs"] > 0, (name, "the persistent kernel did not run (cooperative launch refused?)")
                    assert t["launches_step_water"] == 0 and t["launches_floods_all"] == 0, name
                else:                                      # ... or five launches' (a flood launch per water epoch)
                    assert t["launches_kernel_epochs"] == 0 and t["launches_step_water"] > 0 and t["launches_floods_all"] == t["launches_step_water"], (name, t)
            else:                                          # <= 250 top-level particles: every top-level generation is the tail kernel's from its first epoch
                assert t["launches_kernel_tail"] > 0 and t["epochs_kernel_tail"] > 0, name
            if sets("SMX_RELAX_TAIL_AT", "100000"):       # nested generations of any size too
                assert t["launches_step_water"] == 0 and t["launches_kernel_epochs"] == 0, name
    if engine == "speculative" and sets("SMX_SPEC_MAXNEST", "128"):
        # a sub-phase that commits more than 64 nested particles is cut and re-armed: default64's lakes spawn them by the hundred per phase
        assert doc["scenarios"]["default64"]["counters"]["spec_subphases_cut"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("engine,setting", MATRIX, ids=[setting_id(p) for p in MATRIX])
def test_setting_leaves_results_bit_identical(engine, setting):
    if FIRST_FAULT:
        pytest.fail(f"not started: an earlier child of this module ended in trouble -- {FIRST_FAULT}")
    want = expected(engine)
    doc = run_child(engine, setting)
    check_table(doc["switches"], setting)
    assert sorted(doc["scenarios"]) == sorted(want)
    for name, w in want.items():
        got = doc["scenarios"][name]
        if engine == "lbm":
            for k, (a, b) in enumerate(zip(got["steps"], w["steps"])):
                assert a == b, (name, "step", k, [f for f in a if a[f] != b[f]])
            assert len(got["steps"]) == len(w["steps"]) == sc.LBM_STEPS + 1
            assert got["moved"] == w["moved"], (name, "tracers")
            continue
        assert len(got["hashes"]) == len(w["hashes"])
        for t, (a, b) in enumerate(zip(got["hashes"], w["hashes"])):
            assert a == b, (name, "tick", t + 1, [f for f in a if a[f] != b[f]])
        assert {k: got["counters"][k] for k in w["counters"]} == w["counters"], name
        if "batch_stats" in w:
            assert got["batch_stats"] == w["batch_stats"], name
        else:
            assert got["batch_stats"]["children_lost"] == 0, name
    check_path(engine, setting, doc)


def test_every_neutral_switch_has_a_setting():
    """completeness (no GPU needed: the table is the library's, the matrix is this module's): every `neutral` switch is moved off its
    default by at least one setting; no exemptions. A switch added later without a setting fails here."""
    from soilmachine_amd import capi
    table = capi.switches()
    moved = set()
    for _, setting in MATRIX:
        for k, v in setting.items():
            assert k in table, f"{k} is no switch of the library"
            assert table[k]["class"] != "changes_results", f"{k} changes results: no equality test can hold"
            if v != table[k]["default"]:
                moved.add(k)
    missing = sorted(k for k, e in table.items() if e["class"] == "neutral" and k not in moved)
    assert not missing, f"neutral switches without a setting in MATRIX: {missing}"
