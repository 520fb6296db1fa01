"""The lake census on a real MI355X (smx_lakes / smx_ensemble_lakes): every record field and the label plane equal the restatement
tests/lakes_ref.py exactly -- floats by their bits -- and equal the same kernel bodies compiled for the host (tests/lakes_host)."""
import ctypes as C

import numpy as np
import pytest

from analysis_host_lib import lakes as H
import lakes_ref as R
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from observe_ref import figures_ref
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def check(m, want, what):
    """m.lakes(labels=True) against (records, labels); returns the records."""
    recs, labels = m.lakes(labels=True)
    R.assert_same_census((recs, labels), want, what)
    assert all(r["volume"] == r["volume_q40"] * 2.0 ** -40 for r in recs)
    return recs


# ---------------------------------------------------------------- 1. the shape inputs
@pytest.mark.parametrize("dims", R.SIZES + [(128, 128)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_shapes_equal_the_restatement_and_the_host_bodies(dims):
    names = sorted(R.SHAPES) if dims != (128, 128) else ["bernoulli41", "spiral", "all", "comb"]     # (128^2: 16 tiles and 32 statistics blocks)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        s, want = R.case(name, dims)
        m.load(s)
        recs = check(m, want, f"{name} {dims}")
        hrecs, hlabels, hn = H.run(s)
        R.assert_same_census((recs, None), (hrecs, None), f"{name} {dims}: device against the host-compiled bodies")
        assert hn == len(recs)
    m.close()


def test_values_and_caps():
    s = R.values_case()                      # unequal levels, a -0.0 size, a size of 2^24, empty columns
    want = R.census(s)
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    recs = check(m, want, "values")
    assert [r["flags"] for r in recs] == [0, 1, 3]
    n = len(recs)
    for cap in (1, n - 1, n, n + 4):
        got, labels = m.lakes(labels=True, cap=cap)
        R.assert_same_census((got, labels), (want[0][:cap], want[1]), f"cap {cap}")
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n, 0xFFFFFFFF, np.uint32)
    cnt = C.c_uint32()
    m._chk(m.L.smx_lakes(m.h, capi.ptr(short), 16, n, C.byref(cnt), None))
    assert cnt.value == n
    for k, r in enumerate(want[0]):
        assert (int(short[4 * k]), int(short[4 * k + 1])) == (r["first_cell"], r["cells"])
        assert int(short[4 * k + 2]) | int(short[4 * k + 3]) << 32 == r["volume_q40"]
    m.close()


# ---------------------------------------------------------------- 2. ticked states
def test_ticked_serial_state_is_the_golden_census():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    recs, labels = sm.map.lakes(labels=True)                 # right behind the ticks
    sm.map.sync()
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    R.assert_same_census((recs, labels), R.census(s), "default64.t20")
    assert len(recs) == 3 and sum(r["cells"] for r in recs) == 399 and max(r["cells"] for r in recs) == 386
    sm.map.close()


def test_ticked_relaxed_state():
    sm = SoilMachine(cfg64(), dimx=96, dimy=80, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6, sync=True)
    s = sm.map.snapshot()
    recs = check(sm.map, R.census(s), "relaxed 96x80")
    assert sum(r["cells"] for r in recs) == figures_ref(s)["wet_cells"]
    sm.map.close()


# ---------------------------------------------------------------- 3. queued work is seen, nothing is changed
def test_census_sees_queued_ticks_and_is_read_only():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 20)
    sm.tick(8, sync=True)
    sm.tick(3)                                               # queued, not waited for
    first = sm.map.lakes(labels=True)
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters())
    again = sm.map.lakes(labels=True)
    R.assert_same_census(first, again, "behind queued ticks against after a sync")
    assert (sm.map.digest(), sm.map.counters()) == before, "the census changed the map or a counter"
    R.assert_same_census(again, R.census(sm.map.snapshot()), "after 11 ticks")
    sm.map.close()


# ---------------------------------------------------------------- 4. an ensemble of mixed dimensions
def test_ensemble_of_mixed_dimensions():
    cfgs = [load_cfg("default.soil"), load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")]
    with Ensemble(0) as ens:
        assert ens.lakes() == [] and ens.lake_counts() == []
        assert ens.L.smx_ensemble_lakes(ens.h, None, 64, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = [ens.add(cfgs[0], 64, 64, seed=4, pool=1 << 18), ens.add(cfgs[1], 48, 80, seed=1, pool=1 << 19), ens.add(cfgs[2], 33, 47, seed=7, pool=1 << 18)]
        ens.tick([120, 90, 60], [0, 40, 30], n=4)
        ens.sync()
        for k, (x, y) in enumerate([(3, 4), (3, 5), (17, 40), (63, 63), (0, 0), (31, 32), (40, 9), (41, 10)]):
            mem[0].add(x, y, 0.004 + 0.0011 * k, 0)          # standing water, whether or not a lake has formed by itself
        mem[1].add(5, 70, 0.02, 0); mem[1].add(47, 79, 0.01, 0)
        mem[2].add(32, 46, 0.03, 0); mem[2].add(10, 10, 0.02, 0); mem[2].add(11, 11, 0.02, 0)
        got = ens.lakes()
        counts = ens.lake_counts()
        for i, m in enumerate(mem):
            want = R.census(m.snapshot())
            own = m.lakes(labels=True)
            R.assert_same_census(own, want, f"member {i} by itself")
            R.assert_same_census((got[i], None), (want[0], None), f"member {i} in the ensemble call")
            assert counts[i] == len(want[0])
        assert counts[0] >= 3 and counts[1] >= 1 and counts[2] >= 1, "a member has more lakes than the cap below"
        # fewer records than one member has lakes: the counts stay, the records are cut, in the caller's layout
        cap = 2
        out = (capi.Lake * (3 * cap))()
        n = np.zeros(3, np.uint32)
        ens._chk(ens.L.smx_ensemble_lakes(ens.h, out, C.sizeof(capi.Lake), cap, capi.ptr(n)))
        assert [int(v) for v in n] == counts
        for i in range(3):
            R.assert_same_census(([out[i * cap + k].as_dict() for k in range(min(cap, counts[i]))], None), (got[i][:cap], None), f"cap 2, member {i}")
        assert [len(x) for x in ens.lakes(cap=1)] == [1, 1, 1]


# ---------------------------------------------------------------- 5. forked members
def test_forked_members():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 18)
    sm.tick(8, sync=True)
    src = sm.map.lakes()
    assert len(src) >= 1
    with Ensemble(0) as ens:
        ens.fork(sm.map, 4, pool=1 << 18)
        got = ens.lakes()
        for i in range(4):
            R.assert_same_census((got[i], None), (src, None), f"fork {i}")
        for i, m in enumerate(ens.members):
            m._chk(m.L.smx_srand(m.h, 100 + i))
        ens.tick(d["nwater"], 0, dowind=False)
        got, figs = ens.lakes(), ens.figures()
        for i in range(4):
            assert sum(r["cells"] for r in got[i]) == figs[i]["wet_cells"], f"member {i}"
    sm.map.close()


# ---------------------------------------------------------------- 6. errors, counting, destroy
def test_errors_and_counting_only():
    L = capi.load()
    n = C.c_uint32(7)
    assert L.smx_lakes(None, None, 64, 0, C.byref(n), None) == -2 and n.value == 7
    assert L.smx_ensemble_lakes(None, None, 64, 0, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_lakes(strip.h, None, 64, 0, C.byref(n), None) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.lakes()
    strip.close()
    s, want = R.case("bernoulli20", (64, 64))
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert L.smx_lakes(m.h, None, 0, 0, C.byref(n), None) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_lakes(m.h, None, 64, 3, C.byref(n), None) == -2, "records asked for, nowhere to put them"
    assert L.smx_lakes(m.h, None, 64, 0, C.byref(n), None) == 0 and n.value == len(want[0]) == 318, "cap 0, out NULL: counting only"
    check(m, want, "after the refused calls")
    m.close()                                                # (the census scratch goes with the context)
    # the device still computes the committed golden state
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(5, sync=True)
    assert not compare(sm.map.snapshot(), golden_snapshot("default64", 5))
    recs = sm.map.lakes()
    assert len(recs) == 3 and sum(r["cells"] for r in recs) == 261 and max(r["cells"] for r in recs) == 258
    sm.map.close()
