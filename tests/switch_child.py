"""Child process of tests/test_gpu_switches.py (and its table of scenarios): every scenario of ONE engine on the device, under
whatever SMX_* switches the parent put into the environment -- the library reads them once per process, so a setting needs a
process of its own. Prints one JSON document: the switch table as this process read it, and per scenario the state after every
tick as common.snapshot_hashes, the counters, the batch statistics and timing() at the end, and the scenario's wall time (LBM: the
hashes of rho / v / f after every step and of the moved tracers).

The launch shape is the environment's alone: smx_set_relax_launch and smx_set_spec_limits are never called here.

    python tests/switch_child.py {speculative|serial|batched|relaxed|lbm}
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- scenarios: the smallest the suite already trusts. (the parent computes what they must give on the CPU) ----
# exact engines: name -> (soil, golden case, seed, with wind, ticks); particle counts from tests/golden/digests.json
EXACT = {
    "rgps64": ("rockgravelpebblessand.soil", "rgps64", 0, True, 10),          # wind
    "default64": ("default.soil", "default64", 0, False, 20),                 # lakes, floods, nested particles
    "rocksand48x80": ("rocksand.soil", "rocksand48x80", 3, True, 5),          # non-square; 80 % 8 == 0, 48 x 80 cells
}
SERIAL = {"default64": EXACT["default64"]}
# batched engine against Oracle.batched_tick: rows 1, 3 and 6 of tests/test_gpu_batched.py::test_device_equals_restated_schedule
#   name -> (soil, golden case, start tick, nwater, nwind, with wind, ticks, dilate)
BATCHED = {
    "rgps64_t0": ("rockgravelpebblessand.soil", "rgps64", 0, 100, 50, True, 3, 0),
    "default64_t20": ("default.soil", "default64", 20, 250, 0, False, 8, 0),
    "rocksand48x80_t5": ("rocksand.soil", "rocksand48x80", 5, 60, 40, True, 3, 0),
}
# relaxed engine: name -> (reference, soil, golden case, start tick, nwater, nwind, with wind, ticks, wind hand-over threshold, wind steps per epoch)
#   "oracle": tests/test_relaxed.py RESTATED against Oracle.relaxed_tick (the wind phase on the exclusive schedule, the engine's default);
#   "hostsim": two of tests/test_relaxed.py CASES against HostSim.relaxed_tick (the wind phase relaxed first: k_relax_step<wind> and the
#   colour lists of a wind epoch)
RELAXED = {
    "o_rgps64_t0": ("oracle", "rockgravelpebblessand.soil", "rgps64", 0, 100, 50, True, 3, 0xFFFFFFFF, 4),
    "o_default64_t20": ("oracle", "default.soil", "default64", 20, 250, 0, False, 6, 0xFFFFFFFF, 4),
    "o_painted64_t5": ("oracle", "painted.soil", "painted64", 5, 100, 50, True, 3, 0xFFFFFFFF, 4),
    "o_rocksand48x80_t5": ("oracle", "rocksand.soil", "rocksand48x80", 5, 60, 40, True, 3, 0xFFFFFFFF, 4),
    "h_rgps64_t3": ("hostsim", "rockgravelpebblessand.soil", "rgps64", 3, 100, 50, True, 2, 20, 4),
    "h_rocksand48x80_t5": ("hostsim", "rocksand.soil", "rocksand48x80", 5, 60, 40, True, 3, 10, 3),
}
# LBM wind against LbmOracle: two awkward lattices and one whose 13 workgroups become 16 by the launch's rounding to a multiple of 8 --
# three whole workgroups of the per-XCD remap (csrc/soil_lbm.h lbm_block) lie past the lattice
LBM = {"33x17x70": (33, 17, 70), "5x4x3": (5, 4, 3), "9x9x40": (9, 9, 40)}
LBM_STEPS = 7
LBM_TRACERS = 500
SCENARIOS = {"speculative": EXACT, "serial": SERIAL, "batched": BATCHED, "relaxed": RELAXED, "lbm": LBM}


def sha(a) -> str:
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lbm_boundary(nx, ny, nz):
    """terrain below a wavy surface (as tests/test_lbm.py terrain_boundary, without its random part)"""
    import numpy as np
    hx = 1 + 0.3 * ny * (1 + 0.5 * (np.sin(np.arange(nx)[:, None] / 5.0) + np.cos(np.arange(nz)[None, :] / 7.0)))
    return (hx[:, None, :] > np.arange(ny)[None, :, None]).astype(np.float32)


def lbm_tracers(nx, ny, nz):
    import numpy as np
    rng = np.random.default_rng(2)
    return (rng.random((LBM_TRACERS, 4)) * np.array([nx - 2, ny - 2, nz - 2, 1]) + np.array([0.5, 0.5, 0.5, 0])).astype(np.float32)


def lbm_run(w, dims, read) -> dict:
    """the LBM scenario on `w` (LbmWind on the device, LbmOracle in the parent; read() -> rho, v, f): hashes after initialize and after
    every step, then the tracers"""
    w.set_boundary(lbm_boundary(*dims)); w.initialize()
    steps = []
    for _ in range(LBM_STEPS + 1):
        r = read()
        steps.append({"rho": sha(r[0]), "v": sha(r[1]), "f": sha(r[2])})
        if len(steps) <= LBM_STEPS:
            w.step(1)
    return {"steps": steps, "moved": sha(w.move(lbm_tracers(*dims)))}


def main(engine: str) -> dict:
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from common import digests, golden_snapshot, load_cfg, snapshot_hashes, case_dims
    from soilmachine_amd import capi
    out = {"engine": engine, "switches": capi.switches(), "scenarios": {}}
    if engine == "lbm":
        from soilmachine_amd.lbm import LbmWind
        for name, dims in LBM.items():
            w, t0 = LbmWind(*dims), time.monotonic()
            res = lbm_run(w, dims, lambda: w.read(f=True))
            res["timing"], res["seconds"] = w.timing(), round(time.monotonic() - t0, 2)
            out["scenarios"][name] = res
            w.close()
        return out
    from soilmachine_amd.machine import Layermap, SoilMachine

    def run(sm, ticks):
        hashes, t0 = [], time.monotonic()
        for _ in range(ticks):
            sm.tick(1, sync=True)
            hashes.append(snapshot_hashes(sm.map.snapshot()))
        res = {"hashes": hashes, "counters": sm.map.counters(), "batch_stats": sm.map.batch_stats(), "timing": sm.map.timing(),
               "seconds": round(time.monotonic() - t0, 2)}
        sm.map.close()
        return res

    def from_golden(cfg, g, eng, nw, nd, wind):
        m = Layermap(cfg, g.dimx, g.dimy, seed=0, initialize=False, engine=eng)
        m.load(g, rand_seed=0)
        sm = SoilMachine.__new__(SoilMachine)
        sm.cfg, sm.map, sm.nwater, sm.nwind, sm.dowater, sm.dowind = cfg, m, nw, nd, True, wind
        return sm

    if engine in ("speculative", "serial"):
        eng = capi.ENGINE_SPECULATIVE if engine == "speculative" else capi.ENGINE_SERIAL
        dig = digests()
        for name, (soil, case, seed, wind, ticks) in SCENARIOS[engine].items():
            cfg = load_cfg(soil)
            d = dig[case]
            dimx, dimy = case_dims(d, cfg)
            sm = SoilMachine(cfg, dimx=dimx, dimy=dimy, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=wind, engine=eng)
            out["scenarios"][name] = run(sm, ticks)
    elif engine == "batched":
        for name, (soil, case, t0, nw, nd, wind, ticks, dilate) in BATCHED.items():
            sm = from_golden(load_cfg(soil), golden_snapshot(case, t0), capi.ENGINE_BATCHED, nw, nd, wind)
            sm.map.set_batch_dilate(dilate)
            out["scenarios"][name] = run(sm, ticks)
    elif engine == "relaxed":
        for name, (_, soil, case, t0, nw, nd, wind, ticks, wmin, wsteps) in RELAXED.items():
            sm = from_golden(load_cfg(soil), golden_snapshot(case, t0), capi.ENGINE_RELAXED, nw, nd, wind)
            sm.map.set_relax_wind(wmin, wsteps)                   # (part of the schedule's definition, not a launch shape)
            out["scenarios"][name] = run(sm, ticks)
    else:
        raise SystemExit(f"unknown engine {engine!r}")
    return out


if __name__ == "__main__":
    doc = main(sys.argv[1])
    print("SWITCH-CHILD-JSON " + json.dumps(doc))
