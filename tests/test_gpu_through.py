"""Through-drainage on a real MI355X (smx_through / smx_ensemble_through): every record field, the count and both planes equal the
restatement tests/through_ref.py exactly -- floats by their bits -- and equal the same kernel bodies compiled for the host
(tests/through_host); the level sweeps and the hop sweeps the call launched stay within the restatement's Jacobi rounds, rounded up
to a batch."""
import ctypes as C

import numpy as np
import pytest

import drainage_ref
import lakes_ref
import spill_ref
import streams_ref
from analysis_host_lib import through as H
import through_ref as R
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
TSZ = C.sizeof(capi.Through)
_maps = {}


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def bound(rounds):
    g = H.batch()
    return -(-rounds // g) * g


def sweeps_ok(sw, extra, what):
    lsw, hsw, batches = sw
    g = H.batch()
    print(f"{what}: {lsw} level sweeps ({extra['level_rounds']} rounds), {hsw} hop sweeps ({extra['hop_rounds']} rounds), {batches} batches")
    assert lsw % g == 0 and hsw % g == 0 and lsw + hsw == batches * g, f"{what}: {lsw} + {hsw} sweeps in {batches} batches"
    assert 0 < lsw <= bound(extra["level_rounds"]), f"{what}: {lsw} level sweeps, {extra['level_rounds']} Jacobi rounds"
    assert 0 < hsw <= bound(extra["hop_rounds"]), f"{what}: {hsw} hop sweeps, {extra['hop_rounds']} Jacobi rounds"


def full(s):
    base = drainage_ref.drainage(s)
    sp = spill_ref.spill(s, base)
    return base, sp, R.through(s, base, sp)


def check(m, s, want, what):
    """m.through with both planes against (records, planes, extra), the invariants against the device's own drainage() and spill(),
    the sweep bounds; returns the records and the planes."""
    recs, planes = m.through(area=True, outlets=True)
    sw = m.through_sweeps()
    R.assert_same_through((recs, planes), want, what)
    R.assert_invariants(s, recs, planes, m.drainage(labels=True, area=True), m.spill(), what)
    sweeps_ok(sw, want[2], what)
    return recs, planes


@pytest.fixture(scope="module")
def maps():
    yield _maps
    for m in _maps.values():
        m.close()
    _maps.clear()


# ---------------------------------------------------------------- 1. the inputs
@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(maps, name, dims):
    if dims not in maps:
        maps[dims] = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    m = maps[dims]
    s, base, sp, want = R.case(name, dims)
    m.load(s)
    got = check(m, s, want, f"{name} {dims}")
    (hrecs, hplanes, hn), _ = H.run(s)
    R.assert_same_through(got, (hrecs, hplanes), f"{name} {dims}: device against the host-compiled bodies", count=hn)
    only = m.through()                                      # records only: the same records
    R.assert_same_through((only, None), want, f"{name} {dims}: records only")
    sweeps_ok(m.through_sweeps(), want[2], f"{name} {dims}: records only")
    one = m.through(area=True)                              # one plane without the other
    assert set(one[1]) == {"through_area"}
    R.assert_same_through(one, want, f"{name} {dims}: the area alone")


def test_caps_and_a_short_struct():
    s, base, sp, want = R.case("random_bernoulli20", (96, 80))
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = len(want[0])
    assert n > 8
    for cap in (1, n - 1, n, n + 4):
        got = m.through(area=True, outlets=True, cap=cap)
        assert len(got[0]) == min(cap, n)
        R.assert_same_through(got, (want[0][:cap], want[1]), f"cap {cap}")
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n + 4, 0xFFFFFFFF, np.uint32)
    cnt = C.c_uint32()
    m._chk(m.L.smx_through(m.h, capi.ptr(short), 16, n, C.byref(cnt), None, None))
    assert cnt.value == n and (short[4 * n:] == 0xFFFFFFFF).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["exit_cell"], r["exit_to"], r["down"]]
    m.close()


# ---------------------------------------------------------------- 2. ticked states
def test_ticked_serial_state_is_the_golden_through():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    got = sm.map.through(area=True, outlets=True)             # right behind the ticks
    sw = sm.map.through_sweeps()
    sm.map.sync()
    s = sm.map.snapshot()
    gold = golden_snapshot("default64", 20)
    assert not compare(s, gold)
    base, sp, want = full(gold)
    R.assert_same_through(got, want, "default64.t20")
    R.assert_invariants(gold, got[0], got[1], sm.map.drainage(labels=True, area=True), sm.map.spill(), "default64.t20")
    sweeps_ok(sw, want[2], "default64.t20")
    assert sw == (H.batch(), H.batch(), 2)
    assert len(got[0]) == 29 and sum(1 for r in got[0] if r["down"] == R.NONE) == 26 and max(r["hops"] for r in got[0]) == 2
    assert max(r["through_cells"] for r in got[0]) == 2446
    sm.map.close()


def test_ticked_relaxed_state():
    sm = SoilMachine(cfg64(), dimx=96, dimy=80, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6, sync=True)
    s = sm.map.snapshot()
    check(sm.map, s, full(s)[2], "relaxed 96x80")
    sm.map.close()


# ---------------------------------------------------------------- 3. queued work is seen, nothing is changed
def test_through_sees_queued_ticks_and_is_read_only():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 20)
    sm.tick(8, sync=True)
    sm.tick(3)                                               # queued, not waited for
    first = sm.map.through(area=True, outlets=True)
    sm.map.sync()
    planes = dict(receivers=True, labels=True, area=True)
    before = (sm.map.digest(), sm.map.counters())
    drain, lakes, streams = sm.map.drainage(**planes), sm.map.lakes(labels=True), sm.map.streams(4, order=True, segments=True)
    spill = sm.map.spill(filled=True)
    again = sm.map.through(area=True, outlets=True)
    R.assert_same_through(first, again, "behind queued ticks against after a sync")
    assert (sm.map.digest(), sm.map.counters()) == before, "through changed the map or a counter"
    drainage_ref.assert_same_drainage(sm.map.drainage(**planes), drain, "drainage() after through()")
    lakes_ref.assert_same_census(sm.map.lakes(labels=True), lakes, "lakes() after through()")
    streams_ref.assert_same_streams(sm.map.streams(4, order=True, segments=True), streams, "streams() after through()")
    spill_ref.assert_same_spill(sm.map.spill(filled=True), spill, "spill() after through()")
    R.assert_same_through(again, full(sm.map.snapshot())[2], "after 11 ticks")
    sm.map.close()


# ---------------------------------------------------------------- 4. an ensemble of mixed dimensions
def test_ensemble_of_mixed_dimensions():
    cfgs = [load_cfg("default.soil"), load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")]
    with Ensemble(0) as ens:
        assert ens.through() == []
        assert ens.L.smx_ensemble_through(ens.h, None, TSZ, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = [ens.add(cfgs[0], 64, 64, seed=4, pool=1 << 18), ens.add(cfgs[1], 48, 80, seed=1, pool=1 << 19), ens.add(cfgs[2], 33, 47, seed=7, pool=1 << 18)]
        ens.tick([120, 90, 60], [0, 40, 30], n=4)
        ens.sync()
        for k, (x, y) in enumerate([(3, 4), (3, 5), (17, 40), (63, 63), (0, 0), (31, 32)]):
            mem[0].add(x, y, 0.004 + 0.0011 * k, 0)          # standing water, whether or not a lake has formed by itself
        mem[1].add(5, 70, 0.02, 0); mem[2].add(32, 46, 0.03, 0)
        got = ens.through()
        sw = ens.through_sweeps()
        extra = {"level_rounds": 0, "hop_rounds": 0}
        for i, m in enumerate(mem):
            s = m.snapshot()
            want = full(s)[2]
            extra = {k: max(extra[k], want[2][k]) for k in extra}
            check(m, s, want, f"member {i} by itself")
            R.assert_same_through((got[i], None), want, f"member {i} in the ensemble call")
        sweeps_ok(sw, extra, "the ensemble call")
        assert min(len(g) for g in got) > 2, "every member has more basins than the cap below"
        # fewer records than a member has basins: the counts stay, the records are cut, in the caller's layout
        cap = 2
        out = (capi.Through * (3 * cap))()
        n = np.zeros(3, np.uint32)
        ens._chk(ens.L.smx_ensemble_through(ens.h, out, TSZ, cap, capi.ptr(n)))
        assert [int(v) for v in n] == [len(g) for g in got] == ens.basin_counts()
        for i in range(3):
            R.assert_same_through(([out[i * cap + k].as_dict() for k in range(cap)], None), (got[i][:cap], None), f"cap 2, member {i}")
        assert [len(x) for x in ens.through(cap=1)] == [1, 1, 1]


# ---------------------------------------------------------------- 5. errors, counting
def test_errors_and_counting_only():
    L = capi.load()
    n = C.c_uint32(7)
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert L.smx_through(None, None, TSZ, 0, C.byref(n), None, None) == -2 and n.value == 7
    assert L.smx_ensemble_through(None, None, TSZ, 0, None) == -2
    assert L.smx_get_through_sweeps(None, C.byref(a), C.byref(b), C.byref(c)) == -2
    assert L.smx_ensemble_get_through_sweeps(None, C.byref(a), C.byref(b), C.byref(c)) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_through(strip.h, None, TSZ, 0, C.byref(n), None, None) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.through()
    strip.close()
    s, base, sp, want = R.case("random_bernoulli20", (64, 64))
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert m.through_sweeps() == (0, 0, 0)
    assert L.smx_through(m.h, None, 0, 0, C.byref(n), None, None) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_through(m.h, None, TSZ, 0, None, None, None) == -2 and b"nbasins is null" in L.smx_last_error(m.h)
    assert L.smx_through(m.h, None, TSZ, 3, C.byref(n), None, None) == -2 and b"out is null" in L.smx_last_error(m.h), "records asked for, nowhere to put them"
    assert L.smx_get_through_sweeps(m.h, None, C.byref(b), C.byref(c)) == -2 and L.smx_get_through_sweeps(m.h, C.byref(a), C.byref(b), None) == -2
    assert n.value == 7
    assert L.smx_through(m.h, None, TSZ, 0, C.byref(n), None, None) == 0 and n.value == len(want[0]), "cap 0, out NULL: counting only"
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        assert L.smx_ensemble_through(ens.h, None, 0, 0, capi.ptr(np.zeros(1, np.uint32))) == -2 and b"struct_size" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_through(ens.h, None, TSZ, 0, None) == -2 and b"nbasins is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_through(ens.h, None, TSZ, 2, capi.ptr(np.zeros(1, np.uint32))) == -2 and b"out is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_get_through_sweeps(ens.h, C.byref(a), None, C.byref(c)) == -2
        assert [len(g) for g in ens.through()] == [len(e.through())]
    check(m, s, want, "random_bernoulli20 after the refused calls")
    # the census, the drainage and the spill analysis on the same context are what they were: their scratch is their own
    lakes_ref.assert_same_census(m.lakes(labels=True), lakes_ref.census(s), "smx_lakes after the through calls")
    drainage_ref.assert_same_drainage(m.drainage(receivers=True, labels=True, area=True), base, "smx_drainage after the through calls")
    spill_ref.assert_same_spill(m.spill(filled=True), sp, "smx_spill after the through calls")
    m.close()                                                # (the through scratch goes with the context)
