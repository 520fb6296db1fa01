"""Drainage on a real MI355X (smx_drainage / smx_ensemble_drainage): every record field, the count and the three planes equal the
restatement tests/drainage_ref.py exactly -- floats by their bits -- and equal the same kernel bodies compiled for the host
(tests/drainage_host)."""
import ctypes as C

import numpy as np
import pytest

from analysis_host_lib import drainage as H
import drainage_ref as R
import lakes_ref
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
ALL = dict(receivers=True, labels=True, area=True)
BSZ = C.sizeof(capi.Basin)


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def check(m, s, want, what):
    """m.drainage with all three planes against (records, planes) and the invariants, the lakes taken from smx_lakes; returns the
    records and the planes."""
    recs, planes = m.drainage(**ALL)
    R.assert_same_drainage((recs, planes), want, what)
    R.assert_invariants(s, recs, planes, lakes=m.lakes(), what=what)
    assert not (planes["labels"] == 0xFFFFFFFF).any()
    return recs, planes


# ---------------------------------------------------------------- 1. the inputs
@pytest.mark.parametrize("dims", R.SIZES + [R.BIG], ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(dims):
    names = sorted(R.INPUTS) if dims != R.BIG else R.BIG_INPUTS           # (128^2: 16 tiles and 32 statistics blocks)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        s, want = R.case(name, dims)
        m.load(s)
        got = check(m, s, want, f"{name} {dims}")
        hrecs, hplanes, hn = H.run(s)
        R.assert_same_drainage(got, (hrecs, hplanes), f"{name} {dims}: device against the host-compiled bodies")
        assert hn == len(got[0])
        # records only, and one plane at a time: the same records, the same plane
        assert not any(R.same(a, b) for a, b in zip(m.drainage(), want[0])) and len(m.drainage()) == len(want[0])
        for p in R.PLANES:
            R.assert_same_drainage(m.drainage(**{p: True}), want, f"{name} {dims}: {p} alone")
    m.close()


def test_caps_and_a_short_struct():
    s, want = R.case("random_bernoulli20", (96, 80))
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = len(want[0])
    assert n > 8
    for cap in (1, n - 1, n, n + 4):
        got = m.drainage(cap=cap, **ALL)
        assert len(got[0]) == min(cap, n)
        R.assert_same_drainage(got, (want[0][:cap], want[1]), f"cap {cap}")
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n + 4, 0xFFFFFFFF, np.uint32)
    cnt = C.c_uint32()
    m._chk(m.L.smx_drainage(m.h, capi.ptr(short), 16, n, C.byref(cnt), None, None, None))
    assert cnt.value == n and (short[4 * n:] == 0xFFFFFFFF).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["cells"], r["wet_cells"], r["flags"]]
    m.close()


# ---------------------------------------------------------------- 2. ticked states
def test_ticked_serial_state_is_the_golden_drainage():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    got = sm.map.drainage(**ALL)                               # right behind the ticks
    sm.map.sync()
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    want = R.drainage(s)
    R.assert_same_drainage(got, want, "default64.t20")
    R.assert_invariants(s, got[0], got[1], lakes=sm.map.lakes(), what="default64.t20")
    # the figures of the restatement
    recs, _, extra = want
    lake = [r for r in recs if r["flags"] & R.F_LAKE]
    dry = [r for r in recs if not r["flags"] & R.F_LAKE]
    assert len(lake) == 3 and len(dry) == 26 and all(r["flags"] & R.F_BORDER for r in dry)
    assert sum(r["cells"] for r in lake) == 1843 and int(extra["steps"].max()) == 54
    sm.map.close()


def test_ticked_relaxed_state():
    sm = SoilMachine(cfg64(), dimx=96, dimy=80, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6, sync=True)
    s = sm.map.snapshot()
    check(sm.map, s, R.drainage(s), "relaxed 96x80")
    sm.map.close()


# ---------------------------------------------------------------- 3. queued work is seen, nothing is changed
def test_drainage_sees_queued_ticks_and_is_read_only():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 20)
    sm.tick(8, sync=True)
    sm.tick(3)                                               # queued, not waited for
    first = sm.map.drainage(**ALL)
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters())
    again = sm.map.drainage(**ALL)
    R.assert_same_drainage(first, again, "behind queued ticks against after a sync")
    assert (sm.map.digest(), sm.map.counters()) == before, "drainage changed the map or a counter"
    R.assert_same_drainage(again, R.drainage(sm.map.snapshot()), "after 11 ticks")
    sm.map.close()


# ---------------------------------------------------------------- 4. an ensemble of mixed dimensions
def test_ensemble_of_mixed_dimensions():
    cfgs = [load_cfg("default.soil"), load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")]
    with Ensemble(0) as ens:
        assert ens.drainage() == [] and ens.basin_counts() == []
        assert ens.L.smx_ensemble_drainage(ens.h, None, BSZ, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = [ens.add(cfgs[0], 64, 64, seed=4, pool=1 << 18), ens.add(cfgs[1], 48, 80, seed=1, pool=1 << 19), ens.add(cfgs[2], 33, 47, seed=7, pool=1 << 18)]
        ens.tick([120, 90, 60], [0, 40, 30], n=4)
        ens.sync()
        for k, (x, y) in enumerate([(3, 4), (3, 5), (17, 40), (63, 63), (0, 0), (31, 32)]):
            mem[0].add(x, y, 0.004 + 0.0011 * k, 0)          # standing water, whether or not a lake has formed by itself
        mem[1].add(5, 70, 0.02, 0); mem[2].add(32, 46, 0.03, 0)
        got = ens.drainage()
        counts = ens.basin_counts()
        for i, m in enumerate(mem):
            s = m.snapshot()
            want = R.drainage(s)
            own = check(m, s, want, f"member {i} by itself")
            R.assert_same_drainage((got[i], None), want, f"member {i} in the ensemble call", count=counts[i])
        assert min(counts) > 2, "every member has more basins than the cap below"
        # fewer records than a member has basins: the counts stay, the records are cut, in the caller's layout
        cap = 2
        out = (capi.Basin * (3 * cap))()
        n = np.zeros(3, np.uint32)
        ens._chk(ens.L.smx_ensemble_drainage(ens.h, out, BSZ, cap, capi.ptr(n)))
        assert [int(v) for v in n] == counts
        for i in range(3):
            R.assert_same_drainage(([out[i * cap + k].as_dict() for k in range(cap)], None), (got[i][:cap], None), f"cap 2, member {i}")
        assert [len(x) for x in ens.drainage(cap=1)] == [1, 1, 1]


# ---------------------------------------------------------------- 5. forked members
def test_forked_members():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 18)
    sm.tick(8, sync=True)
    src = sm.map.drainage()
    assert len(src) >= 1
    with Ensemble(0) as ens:
        ens.fork(sm.map, 4, pool=1 << 18)
        got = ens.drainage()
        for i in range(4):
            R.assert_same_drainage((got[i], None), (src, None), f"fork {i}")
            R.assert_same_drainage(ens.members[i].drainage(**ALL), sm.map.drainage(**ALL), f"fork {i} by itself")
    sm.map.close()


# ---------------------------------------------------------------- 6. errors, counting
def test_errors_and_counting_only():
    L = capi.load()
    n = C.c_uint32(7)
    assert L.smx_drainage(None, None, BSZ, 0, C.byref(n), None, None, None) == -2 and n.value == 7
    assert L.smx_ensemble_drainage(None, None, BSZ, 0, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_drainage(strip.h, None, BSZ, 0, C.byref(n), None, None, None) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.drainage()
    strip.close()
    s, want = R.case("random_bernoulli20", (64, 64))
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert L.smx_drainage(m.h, None, 0, 0, C.byref(n), None, None, None) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_drainage(m.h, None, BSZ, 0, None, None, None, None) == -2 and b"nbasins is null" in L.smx_last_error(m.h)
    assert L.smx_drainage(m.h, None, BSZ, 3, C.byref(n), None, None, None) == -2 and b"out is null" in L.smx_last_error(m.h), "records asked for, nowhere to put them"
    assert n.value == 7
    assert L.smx_drainage(m.h, None, BSZ, 0, C.byref(n), None, None, None) == 0 and n.value == len(want[0]), "cap 0, out NULL: counting only"
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        assert L.smx_ensemble_drainage(ens.h, None, 0, 0, capi.ptr(np.zeros(1, np.uint32))) == -2 and b"struct_size" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_drainage(ens.h, None, BSZ, 0, None) == -2 and b"nbasins is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_drainage(ens.h, None, BSZ, 2, capi.ptr(np.zeros(1, np.uint32))) == -2 and b"out is null" in L.smx_ensemble_last_error(ens.h)
        assert ens.basin_counts() == [len(e.drainage())]
    check(m, s, want, "after the refused calls")
    # the census on the same context is what it was: its scratch is its own
    lakes_ref.assert_same_census(m.lakes(labels=True), lakes_ref.census(s), "smx_lakes after the drainage calls")
    m.close()                                                # (the drainage scratch goes with the context)
