"""The stream network on a real MI355X (smx_streams / smx_ensemble_streams): every record field, the count and the four planes equal
the restatement tests/streams_ref.py exactly -- doubles by their bits -- and equal the same kernel bodies compiled for the host
(tests/streams_host)."""
import ctypes as C

import numpy as np
import pytest

import drainage_ref as D
import lakes_ref
from analysis_host_lib import streams as H
import streams_ref as R
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
ALL = dict(order=True, segments=True, reach=True, heads=True)
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
SSZ = C.sizeof(capi.Stream)


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def check(m, s, threshold, want, what, drain=None):
    """m.streams with all four planes against (records, planes) and the invariants; returns the records and the planes."""
    recs, planes = m.streams(threshold, **ALL)
    R.assert_same_streams((recs, planes), want, what)
    R.assert_invariants(s, threshold, recs, planes, drain=drain, what=what)
    return recs, planes


# ---------------------------------------------------------------- 1. the inputs
@pytest.mark.parametrize("dims", D.SIZES + [D.BIG], ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(dims):
    names = sorted(D.INPUTS) if dims != D.BIG else D.BIG_INPUTS           # (128^2: many tiles and several scan blocks)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        m.load(D.case(name, dims)[0])
        for t in R.THRESHOLDS:
            s, drain, want = R.case(name, dims, t)
            what = f"{name} {dims} threshold {t}"
            got = check(m, s, t, want, what, drain)
            hrecs, hplanes, hn = H.run(s, t)
            R.assert_same_streams(got, (hrecs, hplanes), f"{what}: device against the host-compiled bodies")
            assert hn == len(got[0])
            # records only, and one plane at a time: the same records, the same plane
            only = m.streams(t)
            assert len(only) == len(want[0]) and not any(R.same(a, b) for a, b in zip(only, want[0]))
            if t == 3:
                for p in R.PLANES:
                    R.assert_same_streams(m.streams(t, **{p: True}), want, f"{what}: {p} alone")
    m.close()


def test_zero_records_and_the_long_walk():
    m = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    s, drain, want = R.case("plateau", (64, 64), 8)
    m.load(s)
    recs, planes = m.streams(8, **ALL)
    assert recs == [] and want[0] == [] and (planes["segments"] == 0xFFFFFFFF).all() and not planes["order"].any()
    s, drain, want = R.case("spiral", (64, 64), 8)                         # one segment of 2040 cells
    m.load(s)
    recs, planes = check(m, s, 8, want, "spiral 64x64 threshold 8", drain)
    assert len(recs) == 1 and recs[0]["cells"] == 2040 and int(planes["reach"].max()) == 2040
    m.close()


def test_hand_built_network():
    m = Layermap(cfg64(), 16, 16, seed=0, pool=POOL, initialize=False)
    for t in (1, 2, 3):
        s, drain, want = R.hand_case(t)
        m.load(s)
        got = check(m, s, t, want, f"hand-built, threshold {t}", drain)
        R.assert_same_streams(got, H.run(s, t)[:2], f"hand-built, threshold {t}: device against the host-compiled bodies")
    assert len(R.hand_case(1)[2][0]) == 22
    m.close()


def test_caps_and_a_short_struct():
    s, drain, want = R.case("random_bernoulli20", (96, 80), 3)
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5):
        got = m.streams(3, cap=cap, **ALL)
        assert len(got[0]) == min(cap, n)
        R.assert_same_streams(got, (want[0][:cap], want[1]), f"cap {cap}")
        got = m.streams(3, cap=cap, order=True, reach=True, heads=True)     # (without the segments plane the cut segments are not walked)
        R.assert_same_streams(got, (want[0][:cap], want[1]), f"cap {cap}, no segments plane")
    cnt = C.c_uint32()
    m._chk(m.L.smx_streams(m.h, 3, None, SSZ, 0, C.byref(cnt), None, None, None, None))
    assert cnt.value == n, "cap 0, out NULL: counting only"
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n + 4, 0xFFFFFFFE, np.uint32)
    m._chk(m.L.smx_streams(m.h, 3, capi.ptr(short), 16, n, C.byref(cnt), None, None, None, None))
    assert cnt.value == n and (short[4 * n:] == 0xFFFFFFFE).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["last_cell"], r["cells"], r["order"]]
    m.close()


# ---------------------------------------------------------------- 2. ticked states
def test_ticked_serial_state_is_the_golden_network():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    got4 = sm.map.streams(4, **ALL)                            # right behind the ticks
    got1 = sm.map.streams(1, **ALL)
    sm.map.sync()
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    drain = D.drainage(s)
    want4, want1 = R.streams(s, 4, drain), R.streams(s, 1, drain)
    R.assert_same_streams(got4, want4, "default64.t20 threshold 4")
    R.assert_same_streams(got1, want1, "default64.t20 threshold 1")
    R.assert_invariants(s, 4, got4[0], got4[1], drain=drain, what="default64.t20 threshold 4")
    R.assert_invariants(s, 1, got1[0], got1[1], drain=drain, what="default64.t20 threshold 1")
    # the figures of the restatement
    assert len(got4[0]) == 573 and R.orders(got4[0]) == {1: 354, 2: 149, 3: 53, 4: 17}
    assert len(got1[0]) == 1861 and max(r["order"] for r in got1[0]) == 5 and int(got1[1]["reach"].max()) == 55
    sm.map.close()


def test_ticked_relaxed_state():
    sm = SoilMachine(cfg64(), dimx=96, dimy=80, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6, sync=True)
    s = sm.map.snapshot()
    drain = D.drainage(s)
    for t in (1, 8):
        check(sm.map, s, t, R.streams(s, t, drain), f"relaxed 96x80 threshold {t}", drain)
    sm.map.close()


# ---------------------------------------------------------------- 3. queued work is seen, nothing is changed
def test_streams_see_queued_ticks_and_are_read_only():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 20)
    sm.tick(8, sync=True)
    sm.tick(3)                                               # queued, not waited for
    first = sm.map.streams(3, **ALL)
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters())
    again = sm.map.streams(3, **ALL)
    R.assert_same_streams(first, again, "behind queued ticks against after a sync")
    assert (sm.map.digest(), sm.map.counters()) == before, "streams changed the map or a counter"
    s = sm.map.snapshot()
    R.assert_same_streams(again, R.streams(s, 3), "after 11 ticks")
    sm.map.close()


def test_drainage_and_lakes_are_what_they_were():
    s, drain, want = R.case("random_bernoulli20", (96, 80), 3)
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    d0, l0 = m.drainage(**DRAIN_ALL), m.lakes(labels=True)
    D.assert_same_drainage(d0, drain, "drainage before")
    check(m, s, 3, want, "streams, first", drain)
    d1, l1 = m.drainage(**DRAIN_ALL), m.lakes(labels=True)
    check(m, s, 1, R.case("random_bernoulli20", (96, 80), 1)[2], "streams, second", drain)
    d2, l2 = m.drainage(**DRAIN_ALL), m.lakes(labels=True)
    for tag, d, l in (("between", d1, l1), ("after", d2, l2)):
        D.assert_same_drainage(d, d0, f"drainage {tag} the streams calls")
        assert d[0] == d0[0] and all(np.array_equal(d[1][p], d0[1][p]) for p in D.PLANES)
        lakes_ref.assert_same_census(l, l0, f"lakes {tag} the streams calls")
        assert l[0] == l0[0] and np.array_equal(l[1], l0[1])
    lakes_ref.assert_same_census(l2, lakes_ref.census(s), "smx_lakes after the streams calls")
    m.close()


# ---------------------------------------------------------------- 4. an ensemble of mixed dimensions
def test_ensemble_of_mixed_dimensions():
    cases = [R.case("random_bernoulli20", (64, 64), 3), R.case("spiral", (33, 47), 3), R.case("ties", (1, 70), 3), R.case("cone", (96, 80), 3),
             R.case("corners", (70, 1), 3)]
    cfg = cfg64()
    with Ensemble(0) as ens:
        assert ens.streams(3) == []
        assert ens.L.smx_ensemble_streams(ens.h, 3, None, SSZ, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = []
        for s, _, _ in cases:
            mem.append(ens.add(cfg, int(s.dimx), int(s.dimy), seed=1, pool=POOL, initialize=False))
            mem[-1].load(s)
        got = ens.streams(3)
        counts = [len(x) for x in got]
        for i, (m, (s, drain, want)) in enumerate(zip(mem, cases)):
            own = check(m, s, 3, want, f"member {i} by itself", drain)
            R.assert_same_streams((got[i], None), want, f"member {i} in the ensemble call")
            R.assert_same_streams((got[i], None), own, f"member {i}: the ensemble call against its own")
        assert max(counts) > 3
        # fewer records than a member has segments: the counts stay, the records are cut, in the caller's layout
        cap = 3
        out = (capi.Stream * (len(mem) * cap))()
        n = np.zeros(len(mem), np.uint32)
        ens._chk(ens.L.smx_ensemble_streams(ens.h, 3, out, SSZ, cap, capi.ptr(n)))
        assert [int(v) for v in n] == counts
        for i in range(len(mem)):
            k = min(cap, counts[i])
            R.assert_same_streams(([out[i * cap + r].as_dict() for r in range(k)], None), (got[i][:cap], None), f"cap 3, member {i}")
        assert [len(x) for x in ens.streams(3, cap=1)] == [min(1, c) for c in counts]
        assert [len(x) for x in ens.streams(8)] == [len(R.case(nm, dm, 8)[2][0]) for nm, dm in
                                                     (("random_bernoulli20", (64, 64)), ("spiral", (33, 47)), ("ties", (1, 70)), ("cone", (96, 80)), ("corners", (70, 1)))]


# ---------------------------------------------------------------- 5. errors
def test_refused_arguments():
    L = capi.load()
    n = C.c_uint32(7)
    assert L.smx_streams(None, 3, None, SSZ, 0, C.byref(n), None, None, None, None) == -2 and n.value == 7
    assert L.smx_ensemble_streams(None, 3, None, SSZ, 0, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_streams(strip.h, 3, None, SSZ, 0, C.byref(n), None, None, None, None) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.streams(3)
    strip.close()
    s, drain, want = R.case("random_bernoulli20", (64, 64), 3)
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert L.smx_streams(m.h, 3, None, 0, 0, C.byref(n), None, None, None, None) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_streams(m.h, 0, None, SSZ, 0, C.byref(n), None, None, None, None) == -2 and b"threshold" in L.smx_last_error(m.h)
    assert L.smx_streams(m.h, 3, None, SSZ, 0, None, None, None, None, None) == -2 and b"nstreams is null" in L.smx_last_error(m.h)
    assert L.smx_streams(m.h, 3, None, SSZ, 3, C.byref(n), None, None, None, None) == -2 and b"out is null" in L.smx_last_error(m.h), "records asked for, nowhere to put them"
    assert n.value == 7
    with pytest.raises(SoilmxError, match="threshold"):
        m.streams(0)
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        one = capi.ptr(np.zeros(1, np.uint32))
        assert L.smx_ensemble_streams(ens.h, 3, None, 0, 0, one) == -2 and b"struct_size" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_streams(ens.h, 0, None, SSZ, 0, one) == -2 and b"threshold" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_streams(ens.h, 3, None, SSZ, 0, None) == -2 and b"nstreams is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_streams(ens.h, 3, None, SSZ, 2, one) == -2 and b"out is null" in L.smx_ensemble_last_error(ens.h)
        assert [len(x) for x in ens.streams(1)] == [len(e.streams(1))]
    check(m, s, 3, want, "after the refused calls", drain)
    m.close()                                                # (the stream scratch goes with the context)
