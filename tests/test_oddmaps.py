"""The device headers run by host threads (tests/hostsim) on maps that no tile size divides (tests/oddmaps.py), every engine against the
oracle: the exact walk and the speculative protocol against the reference-order tick, the batched and the relaxed schedule against
their restatements -- full state after every tick and the counters at the end (the oracle checks every access of its own steps against
the reservation; the host side is held to it through the equal states). This proves the fixture
(wet start, floods, nested particles on every shape) before anything runs it on the device, and brings the relaxed
engine's odd shapes into the suite."""
import ctypes

import numpy as np
import pytest

import oddmaps as om
from hostsim_lib import HostSim, lib
from soilmachine_amd.snapshot import compare
from test_batched import set_dilate

CASES = [pytest.param(w, s, id=f"{w}-{om.shape_id(s)}") for w in om.WORKLOADS for s in om.SHAPES]


def host(workload, shape):
    h = HostSim(om.cfg_of(workload), shape[0], shape[1], pool=om.POOL, seed=om.SEED)
    h.load(om.start(workload, shape), advance_rand=True)
    return h


def schedule_figures():
    """epochs, generations and lost children of the host-sim's throughput schedules since the last call (process-global: read = reset)"""
    st = np.zeros(8, np.uint32)
    lib().hs_batch_stats(st.ctypes.data_as(ctypes.c_void_p))
    return {"epochs": int(st[0]), "generations": int(st[1]), "children_lost": int(st[2])}


def run_against_oracle(workload, shape, schedule, step, keys, dilate=0, generations=0):
    """`step(h, t)` ticks the host side once; -> the host side's counters"""
    snaps, co, st = om.oracle_run(workload, shape, schedule, dilate, generations)
    om.must_be_wet(shape, co)
    assert st["guard_violations"] == 0 and co["pool_overflow"] == 0
    h = host(workload, shape)
    for t in range(om.TICKS):
        step(h, t)
        bad = compare(h.snapshot(), snaps[t])
        assert not bad, f"{workload} {om.shape_id(shape)} {schedule} tick {t}: {bad}"
    ch = h.counters()
    assert {k: ch[k] for k in keys} == {k: co[k] for k in keys}
    assert ch["pool_overflow"] == 0
    return ch


@pytest.mark.parametrize("workload,shape", CASES)
def test_exact_walk_equals_the_oracle(workload, shape):
    _, nw, nd, wind = om.WORKLOADS[workload]
    run_against_oracle(workload, shape, "exact", lambda h, t: h.tick(nw, nd, True, wind), om.KEYS)


# engine mode 3: blocked filter + suspend/resume; 7: the same through the wave-loop structure of soil_coop.h
@pytest.mark.parametrize("mode,team,shuffle", [(3, 5, 11), (7, 1, 5)], ids=["team5", "wave-loop"])
@pytest.mark.parametrize("workload,shape", CASES)
def test_speculative_protocol_equals_the_oracle(workload, shape, mode, team, shuffle):
    _, nw, nd, wind = om.WORKLOADS[workload]
    HostSim.set_boundary_threads(team)
    try:
        run_against_oracle(workload, shape, "exact",
                           lambda h, t: h.spec_tick(nw, nd, True, wind, nthreads=4, scout=1 | (mode << 4), shuffle=shuffle + t), om.KEYS)
    finally:
        HostSim.set_boundary_threads(1)


@pytest.mark.parametrize("dilate,threads,shuffle", [(0, 1, 0), (1, 3, 7)], ids=["dilate0-1thread", "dilate1-3threads"])
@pytest.mark.parametrize("workload,shape", CASES)
def test_batched_schedule_equals_its_restatement(workload, shape, dilate, threads, shuffle):
    _, nw, nd, wind = om.WORKLOADS[workload]
    _, _, st = om.oracle_run(workload, shape, "batched", dilate)
    set_dilate(dilate)
    try:
        schedule_figures()                                     # (the host-sim's schedule figures are process-global: read = reset)
        run_against_oracle(workload, shape, "batched", lambda h, t: h.batched_tick(nw, nd, True, wind, nthreads=threads, shuffle=shuffle),
                           om.KEYS, dilate)
        hs = schedule_figures()
        assert (hs["epochs"], hs["generations"], hs["children_lost"]) == (st["epochs"], st["generations"], 0)
    finally:
        set_dilate(0)


# the engine's eight water generations, and the whole phase as one (what the device tests put through the dense launches)
@pytest.mark.parametrize("generations,threads,shuffle", [(0, 1, 0), (om.DENSE_GENERATIONS, 3, 5), (om.DENSE_GENERATIONS, 4, 1)],
                         ids=["8gen-1thread", "1gen-3threads-shuffled", "1gen-4threads-shuffled"])
@pytest.mark.parametrize("workload,shape", CASES)
def test_relaxed_schedule_equals_its_restatement(workload, shape, generations, threads, shuffle):
    _, nw, nd, wind = om.WORKLOADS[workload]
    schedule_figures()
    if generations:
        lib().hs_set_water_generations(generations)          # (process-global, like the figures)
    try:
        run_against_oracle(workload, shape, "relaxed",
                           lambda h, t: h.relaxed_tick(nw, nd, True, wind, nthreads=threads, shuffle=shuffle + t if shuffle else 0), om.RKEYS,
                           generations=generations)
    finally:
        lib().hs_reset_water_schedule()
    assert schedule_figures()["children_lost"] == 0
