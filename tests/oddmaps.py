"""Maps that no tile size divides: one fixture recipe, for tests/test_oddmaps.py (host threads) and for device tests of the same cases.

Every other map the suite compares with an independent reference is a multiple of 8 and 16 with a cell count that is a multiple of 64.
The shapes here reach the launch-level code whose indexing depends on the map's shape:

  33x47         both sides odd, cells % 64 != 0 (the last bitmap word of the classification is partial)
  17x19, 9x7    smaller than one 24x24 grid-tile region; 9x7 is 2x1 grid tiles
  23x25         one cell on either side of the region size
  65x63         one cell on either side of every power-of-two tile
  1x70, 70x1    no x-neighbours / no y-neighbours
  64x8, 8x64    the eight-cell classification at its smallest (dimy == 8: a block covers more cells than the map has), and its refusal

The start state is wet (standing water, saturated sections), the judge is the oracle (oracle/soil_oracle.cpp): its exact tick, its batched
schedule and its relaxed schedule, one run per (workload, shape, schedule) shared by every variant that is compared with it."""
from __future__ import annotations

import os

from common import SOILS, load_cfg
from oracle_lib import Oracle, run_ref
from soilmachine_amd.snapshot import read_snapshot, write_snapshot

SHAPES = [(33, 47), (17, 19), (23, 25), (65, 63), (9, 7), (1, 70), (70, 1), (64, 8), (8, 64)]
# the order of a device run: the friendliest shape first, the most degenerate ones last
DEVICE_ORDER = [(65, 63), (33, 47), (23, 25), (17, 19), (64, 8), (8, 64), (1, 70), (70, 1), (9, 7)]

WORKLOADS = {
    # name: soil file, water particles, wind particles, wind on
    "default": ("default.soil", 600, 0, False),                    # 600 > the 256-particle tail threshold: dense kernels, then the tail
    "rgps": ("rockgravelpebblessand.soil", 300, 80, True),
}
TICKS = 3
SEED = 3
# The throughput engines split a water phase into eight generations by default: 75 and 38 particles here, so every epoch of the relaxed
# engine's default launch shape runs in the one-workgroup tail kernel (256 running particles and fewer), and no nested generation of
# these maps is larger. ONE generation puts the whole phase (600, 300) through the dense launches first, then the tail.
DENSE_GENERATIONS = 1
POOL = 1 << 18          # sections per context (every side the same: pool_free is compared); the largest map has 4 095 cells

KEYS = ["steps_water_top", "steps_water_all", "steps_wind", "nested_particles", "floods", "cascade_calls", "cascade_transfers",
        "wcascade_calls", "rand_calls", "pool_free"]
RKEYS = KEYS[:-1]

_cfg, _wet, _runs = {}, {}, {}


def shape_id(shape) -> str:
    return f"{shape[0]}x{shape[1]}"


def cfg_of(workload: str):
    if workload not in _cfg:
        _cfg[workload] = load_cfg(WORKLOADS[workload][0])
    return _cfg[workload]


def wet_state(cfg, dx: int, dy: int):
    """The start state: ten ticks of 250 water particles in the reference's order from the initial terrain, then twelve puddles."""
    o = Oracle(cfg, dx, dy, pool=POOL, seed=SEED)
    o.initialize()
    for _ in range(10):
        o.tick(250, 0, True, False)
    for k in range(12):
        o.L.so_add(o.h, (7 * k + 3) % dx, (11 * k + 5) % dy, 0.01 + 0.004 * k, 0)
    return o.snapshot()


def start(workload: str, shape):
    """the wet start state of (workload, shape): computed once, never changed"""
    key = (workload, shape)
    if key not in _wet:
        _wet[key] = wet_state(cfg_of(workload), *shape)
    return _wet[key]


def fresh_oracle(workload: str, shape) -> Oracle:
    """An oracle loaded FROM THE SNAPSHOT, like every other side: the sticky "has held a saturation" bit of a column is context
    state that a snapshot does not carry (it is derived again on import), and the grid pass's active set depends on it."""
    o = Oracle(cfg_of(workload), shape[0], shape[1], pool=POOL, seed=SEED)
    o.load(start(workload, shape))
    return o


def oracle_run(workload: str, shape, schedule: str = "exact", dilate: int = 0, generations: int = 0):
    """TICKS ticks of the oracle from the wet start -> ([snapshot after every tick], counters, batched stats). `schedule`: "exact" (the
    reference's particle order), "batched" (with `dilate`) or "relaxed"; `generations`: smx_set_water_generations of the two throughput
    schedules (0: their default, eight). Cached: variants of one case share one run."""
    key = (workload, shape, schedule, dilate, generations)
    if key not in _runs:
        _, nw, nd, wind = WORKLOADS[workload]
        o = fresh_oracle(workload, shape)
        if schedule == "batched":
            o.batched_set_dilate(dilate)
        if generations:
            o.L.so_set_water_generations(o.h, generations)
        tick = {"exact": o.tick, "batched": o.batched_tick, "relaxed": o.relaxed_tick}[schedule]
        snaps = []
        for _ in range(TICKS):
            tick(nw, nd, True, wind)
            snaps.append(o.snapshot())
        _runs[key] = (snaps, o.counters(), o.batched_stats())
        o.close()
    return _runs[key]


def ref_run(workload: str, shape, tmpdir: str):
    """the compiled reference (oracle/_ref/soil_ref) continued from the wet start for TICKS ticks -> its last state"""
    soil, nw, nd, wind = WORKLOADS[workload]
    path = os.path.join(tmpdir, "start.snap")
    write_snapshot(path, start(workload, shape))
    run_ref(os.path.join(SOILS, soil), seed=SEED, sizex=shape[0], sizey=shape[1], ticks=TICKS, nwater=nw, nwind=nd, wind=wind, pool=POOL,
            load=path, dump_prefix=os.path.join(tmpdir, "r"), dump_at=[TICKS])
    return read_snapshot(os.path.join(tmpdir, f"r.t{TICKS}.snap"))


def must_be_wet(shape, counters: dict):
    """The condition the fixture has to meet (from the oracle's own counters, not a measurement of the code under test): nested
    particles on every shape, floods wherever both sides are at least 7 cells."""
    assert counters["nested_particles"] > 0, (shape, counters)
    if min(shape) >= 7:
        assert counters["floods"] > 0, (shape, counters)
