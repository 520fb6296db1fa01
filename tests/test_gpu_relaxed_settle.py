"""What follows apply in a dense relaxed epoch, as ONE dataflow launch (k_relax_settle, smx_set_relax_settle mode 1) and as two (k_relax_filter +
k_relax_cascade_flow, mode 0): both against the same headers run by host threads -- full state after every tick and the counters. The per-phase
launches run down to the last particle (set_relax_launch(0, 0)), so every epoch of every generation goes through the launch under test. Shapes: the
smallest at which it can go wrong -- crowding (nearly every flagged cell waits), more than one wavefront, a ragged last one, map edges, a non-square
map, mixed soil types, relaxed wind (two entries per step, rstride entries per particle)."""
import pytest

from common import golden_snapshot, load_cfg
from hostsim_lib import HostSim
from soilmachine_amd import capi
from soilmachine_amd.machine import Layermap, SoilMachine
from soilmachine_amd.snapshot import compare
from test_gpu_relaxed import KEYS

pytestmark = pytest.mark.gpu

SCENES = {
    # soil, golden case, start tick, nwater, nwind, ticks, wind hand-over threshold, wind steps per epoch
    "standing-water": ("default.soil", "default64", 20, 2021, 0, 3, 0, 1),              # half the cells flagged per epoch, floods and nested generations in between
    "non-square-wind": ("rocksand.soil", "rocksand48x80", 5, 700, 300, 2, 0, 3),        # edge clamps of the two scans; relaxed wind, 3 steps per epoch
    "four-soils-wind": ("rockgravelpebblessand.soil", "rgps64", 3, 1500, 500, 2, 0, 1),  # the mixed-type branch of cascade_precheck; relaxed wind, 1 step per epoch
}
_host = {}


def host_states(scene):
    """the host-thread side: one run per scene, shared by every test of it and left unchanged -> ([snapshot per tick], counters)"""
    if scene not in _host:
        soil, case, t0, nw, nd, ticks, wmin, wsteps = SCENES[scene]
        cfg = load_cfg(soil)
        g = golden_snapshot(case, t0)
        h = HostSim(cfg, g.dimx, g.dimy, seed=0)
        h.load(g, advance_rand=True)
        snaps = []
        for t in range(ticks):
            h.relaxed_tick(nw, nd, True, nd > 0, nthreads=4, shuffle=t + 1, wind_min=wmin, wind_steps=wsteps)
            snaps.append(h.snapshot())
        _host[scene] = (snaps, h.counters())
    return _host[scene]


def device(scene, mode, max_waves=0):
    soil, case, t0, nw, nd, ticks, wmin, wsteps = SCENES[scene]
    cfg = load_cfg(soil)
    g = golden_snapshot(case, t0)
    m = Layermap(cfg, g.dimx, g.dimy, seed=0, initialize=False, engine=capi.ENGINE_RELAXED)
    m.load(g, rand_seed=0)
    m.set_relax_wind(wmin, wsteps)
    m.set_relax_launch(0, 0)
    m.set_relax_settle(mode, max_waves)
    sm = SoilMachine.__new__(SoilMachine)
    sm.cfg, sm.map, sm.nwater, sm.nwind, sm.dowater, sm.dowind = cfg, m, nw, nd, True, nd > 0
    return sm, ticks


def run_against_host(scene, mode, max_waves=0):
    """-> the getter's figures after every tick"""
    snaps, ch = host_states(scene)
    sm, ticks = device(scene, mode, max_waves)
    stats = []
    for t in range(ticks):
        sm.tick(1, sync=True)
        bad = compare(sm.map.snapshot(), snaps[t])
        assert not bad, f"{scene} mode {mode} tick {t}: {bad}"
        stats.append(sm.map.relax_settle_stats())
    cd = sm.map.counters()
    assert {k: cd[k] for k in KEYS} == {k: ch[k] for k in KEYS}
    assert sm.map.batch_stats()["children_lost"] == 0
    sm.map.close()
    return stats


@pytest.mark.parametrize("scene", list(SCENES))
def test_the_fused_launch_equals_host_threads(scene):
    stats = run_against_host(scene, 1)
    print("[settle]", scene, stats)
    assert stats[-1]["crowded_cells"] > 0 and stats[-1]["epochs_fused"] > 0, stats     # the scene reached the waiting path
    assert stats[-1]["epochs_split"] == 0, stats                                         # ... and nothing fell back silently
    again = run_against_host(scene, 1)
    assert [s["crowded_cells"] for s in again] == [s["crowded_cells"] for s in stats]   # the path taken is a function of the input


@pytest.mark.parametrize("scene", list(SCENES))
def test_the_two_launches_equal_host_threads(scene):
    stats = run_against_host(scene, 0)
    assert stats[-1]["epochs_split"] > 0 and stats[-1]["epochs_fused"] == 0 and stats[-1]["crowded_cells"] == 0, stats


def test_an_epoch_whose_grid_is_not_resident_takes_the_two_launches():
    """mode 1 on a context that may count on ONE resident wavefront (the setter's cap): every epoch with more than 64 flagged cells in the
    worst case takes the two-launch path -- the fall-back decision, without a large map"""
    stats = run_against_host("standing-water", 1, max_waves=1)
    assert stats[-1]["epochs_split"] > 0, stats                           # (uncapped, the same scene takes none: test_the_fused_launch_equals_host_threads)
