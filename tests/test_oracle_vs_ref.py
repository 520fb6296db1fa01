"""Oracle restatement <-> the compiled reference (oracle/_ref/soil_ref).

The restatement is held to the reference's states stored under tests/golden (restatement_ref.json, written by
tests/golden/make_golden_restatement.py from the compiled reference) everywhere, and live against the binary where
build() produced it. The resume test checks the reference driver itself and needs the binary."""
import os
import tempfile

import pytest

import oddmaps as om
from common import (RESTATEMENT_CASES, RESTATEMENT_ODD_CASES, SOILS, load_cfg, restatement_case_id, restatement_golden,
                    restatement_odd_case_id, restatement_wet_case_id, snapshot_hashes)
from oracle_lib import Oracle, have_ref, run_ref
from soilmachine_amd.snapshot import compare, read_snapshot


@pytest.mark.parametrize("soil,size,seed,ticks,nwater,nwind", RESTATEMENT_CASES)
def test_restatement_equals_reference(soil, size, seed, ticks, nwater, nwind):
    want = restatement_golden()[restatement_case_id(soil, size, seed, ticks, nwater, nwind)]
    cfg = load_cfg(soil)
    o = Oracle(cfg, size, size, seed=seed)
    o.initialize()
    s0 = o.snapshot()
    for _ in range(ticks):
        o.tick(nwater, nwind, True, nwind > 0)
    s1 = o.snapshot()
    if have_ref():                                  # live: the binary's own states, with compare's itemised differences
        with tempfile.TemporaryDirectory() as td:
            run_ref(os.path.join(SOILS, soil), seed=seed, size=size, ticks=ticks, nwater=nwater, nwind=nwind,
                    wind=nwind > 0, dump_prefix=os.path.join(td, "r"), dump_at=[0, ticks])
            r0 = read_snapshot(os.path.join(td, "r.t0.snap"))
            r1 = read_snapshot(os.path.join(td, f"r.t{ticks}.snap"))
        assert not compare(s0, r0)
        assert not compare(s1, r1)
    assert snapshot_hashes(s0) == want["t0"]
    assert snapshot_hashes(s1) == want["end"]


@pytest.mark.parametrize("soil,dimx,dimy,seed,ticks,nwater,nwind", RESTATEMENT_ODD_CASES)
def test_restatement_equals_reference_on_odd_maps(soil, dimx, dimy, seed, ticks, nwater, nwind):
    """the same from the initial terrain on maps that no tile size divides, down to one cell in width (tests/oddmaps.py)"""
    want = restatement_golden()[restatement_odd_case_id(soil, dimx, dimy, seed, ticks, nwater, nwind)]
    cfg = load_cfg(soil)
    o = Oracle(cfg, dimx, dimy, seed=seed)
    o.initialize()
    s0 = o.snapshot()
    for _ in range(ticks):
        o.tick(nwater, nwind, True, nwind > 0)
    s1 = o.snapshot()
    if have_ref():
        with tempfile.TemporaryDirectory() as td:
            run_ref(os.path.join(SOILS, soil), seed=seed, sizex=dimx, sizey=dimy, ticks=ticks, nwater=nwater, nwind=nwind,
                    wind=nwind > 0, dump_prefix=os.path.join(td, "r"), dump_at=[0, ticks])
            r0 = read_snapshot(os.path.join(td, "r.t0.snap"))
            r1 = read_snapshot(os.path.join(td, f"r.t{ticks}.snap"))
        assert not compare(s0, r0)
        assert not compare(s1, r1)
    assert snapshot_hashes(s0) == want["t0"]
    assert snapshot_hashes(s1) == want["end"]


@pytest.mark.parametrize("workload,shape", [pytest.param(w, s, id=f"{w}-{om.shape_id(s)}") for w in om.WORKLOADS for s in om.SHAPES])
def test_restatement_equals_reference_from_the_wet_start_of_the_odd_maps(workload, shape):
    """The judge of tests/test_oddmaps.py, judged: the oracle's exact tick from the wet start state of
    tests/oddmaps.py (standing water, floods, nested particles) against the reference continued from the same snapshot."""
    want = restatement_golden()[restatement_wet_case_id(workload, shape)]
    assert snapshot_hashes(om.start(workload, shape)) == want["t0"]           # the recipe itself has not moved
    snaps, counters, _ = om.oracle_run(workload, shape, "exact")
    om.must_be_wet(shape, counters)
    if have_ref():
        with tempfile.TemporaryDirectory() as td:
            bad = compare(snaps[-1], om.ref_run(workload, shape, td))
        assert not bad, bad
    assert snapshot_hashes(snaps[-1]) == want["end"]


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref/soil_ref not built (build() makes it where the reference sources are present)")
def test_reference_driver_resumes_from_a_snapshot_bit_exactly():
    """oracle/ref_driver.cpp --load (what bench.py's cpu_baseline uses to time the CPU path on the GPU line's own state): k ticks, snapshot,
    load, n - k ticks == n ticks uninterrupted -- full state, rand() draws, and the JSON figures the P2 envelope reads."""
    soil = os.path.join(SOILS, "rockgravelpebblessand.soil")
    kw = dict(seed=3, size=96, nwater=300, nwind=120, lean=True)
    with tempfile.TemporaryDirectory() as td:
        whole = run_ref(soil, ticks=9, dump_prefix=os.path.join(td, "w"), dump_at=[4, 9], **kw)
        part = run_ref(soil, ticks=5, load=os.path.join(td, "w.t4.snap"), dump_prefix=os.path.join(td, "p"), dump_at=[5], **kw)
        assert not compare(read_snapshot(os.path.join(td, "p.t5.snap")), read_snapshot(os.path.join(td, "w.t9.snap")))
        for k in ("sumh", "nsec", "typehash", "rand_calls", "next_rand", "standing", "water_volume"):
            assert part[k] == whole[k], k
        # another rand() stream on the same terrain (the P2 control) leaves the terrain alone and changes the run
        base = run_ref(soil, ticks=0, dump_prefix=os.path.join(td, "b"), dump_at=[0], **kw)
        other = run_ref(soil, ticks=9, rand_seed=77, dump_prefix=os.path.join(td, "o"), dump_at=[0], **kw)
        t0, o0 = read_snapshot(os.path.join(td, "b.t0.snap")), read_snapshot(os.path.join(td, "o.t0.snap"))
        o0.rand_calls = t0.rand_calls
        assert not compare(o0, t0) and base["nsec"] == t0.nsec
        assert other["typehash"] != whole["typehash"] or other["sumh"] != whole["sumh"]
