"""The hillslopes on a real MI355X (smx_hillslopes / smx_ensemble_hillslopes): every record field, the count and the five planes
equal the restatement tests/hillslopes_ref.py exactly -- doubles by their bits -- and equal the same kernel bodies compiled for the
host (tests/hillslopes_host)."""
import ctypes as C

import numpy as np
import pytest

import drainage_ref as D
from analysis_host_lib import hillslopes as H
import hillslopes_ref as R
import lakes_ref
import oddmaps
import streams_ref as S
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
ALL = dict(entry=True, hillslope=True, straight=True, diagonal=True, hand=True)
STREAMS_ALL = dict(order=True, segments=True, reach=True, heads=True)
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
HSZ = C.sizeof(capi.Hillslope)
NOPLANES = (None,) * 5


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def check(m, s, threshold, want, what, drain=None, strm=None):
    """m.hillslopes with all five planes against (records, planes) and the invariants; returns the records and the planes."""
    recs, planes = m.hillslopes(threshold, **ALL)
    R.assert_same_hillslopes((recs, planes), want, what)
    R.assert_invariants(s, threshold, recs, planes, drain=drain, strm=strm, what=what)
    assert all(r["hand_sum"] == r["hand_sum_q40"] * 2.0 ** -40 for r in recs)
    return recs, planes


# ---------------------------------------------------------------- 1. the inputs
@pytest.mark.parametrize("dims", D.SIZES + [D.BIG], ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(dims):
    names = sorted(D.INPUTS) if dims != D.BIG else D.BIG_INPUTS           # (128^2: many tiles and several fold blocks)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        m.load(D.case(name, dims)[0])
        for t in R.THRESHOLDS:                                             # 0, 1 and 3 rounds: the result ends in either set of planes
            s, drain, strm, want = R.case(name, dims, t)
            what = f"{name} {dims} threshold {t}"
            got = check(m, s, t, want, what, drain, strm)
            hrecs, hplanes, hn, _ = H.run(s, t)
            R.assert_same_hillslopes(got, (hrecs, hplanes), f"{what}: device against the host-compiled bodies")
            assert hn == len(got[0])
            only = m.hillslopes(t)                                         # records only
            assert len(only) == len(want[0]) and not any(R.same(a, b) for a, b in zip(only, want[0]))
            if t == 3:
                for p in R.PLANES:
                    R.assert_same_hillslopes(m.hillslopes(t, **{p: True}), want, f"{what}: {p} alone")
    m.close()


def test_the_long_path_and_zero_records():
    m = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    s, drain, strm, want = R.case("plateau", (64, 64), 8)
    m.load(s)
    recs, planes = m.hillslopes(8, **ALL)
    assert recs == [] and want[0] == [] and (planes["hillslope"] == R.NONE).all() and not planes["hand"].any() and not planes["straight"].any()
    for t, nrec in ((4096, 1), (4097, 0)):                                 # twelve rounds; one path of 2046 steps
        s, drain, strm, want = R.case("spiral", (64, 64), t)
        m.load(s)
        recs, planes = check(m, s, t, want, f"spiral 64x64 threshold {t}", drain, strm)
        assert len(recs) == nrec and int((planes["straight"] + planes["diagonal"]).max()) == 2046
        if nrec:
            assert recs[0]["cells"] == 4095 and recs[0]["steps_max"] == 2046
        else:
            assert int(((planes["hillslope"] == R.NONE) & (planes["entry"] != np.arange(4096).reshape(64, 64))).sum()) == 4095
    m.close()
    m = Layermap(cfg64(), 128, 128, seed=0, pool=POOL, initialize=False)
    for t, longest in ((64, 63), (1000, 64)):
        s, drain, strm, want = R.case("cone", (128, 128), t)
        m.load(s)
        recs, planes = check(m, s, t, want, f"cone 128x128 threshold {t}", drain, strm)
        assert max(r["steps_max"] for r in recs) == longest
    m.close()


def test_hand_built_network():
    m = Layermap(cfg64(), 16, 16, seed=0, pool=POOL, initialize=False)
    for t in (1, 2, 3):
        s, drain, strm, want = R.hand_case(t)
        m.load(s)
        got = check(m, s, t, want, f"hand-built, threshold {t}", drain, strm)
        R.assert_same_hillslopes(got, H.run(s, t)[:2], f"hand-built, threshold {t}: device against the host-compiled bodies")
    # the records of threshold 3 as tests/test_hillslopes_host.py writes them out by hand: two of them here
    by = {r["first_cell"]: r for r in got[0]}
    r = by[14 * 16 + 14]
    assert (r["cells"], r["steps_max"], r["farthest_cell"], r["straight_sum"], r["diagonal_sum"], r["hand_max"], r["hand_sum_q40"], r["bank_cells"], r["head_cells"]) == \
        (2, 2, 14 * 16 + 12, 3, 0, 2.0, 3 << 40, 1, 2)
    r = by[4 * 16 + 5]
    assert (r["cells"], r["farthest_cell"], r["diagonal_sum"], r["hand_max"], r["head_cells"]) == (1, 5 * 16 + 5, 1, 5.0, 0)
    assert len(got[0]) == 7
    m.close()


def test_caps_and_a_short_struct():
    s, drain, strm, want = R.case("random_bernoulli20", (96, 80), 3)
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5):
        got = m.hillslopes(3, cap=cap, **ALL)
        assert len(got[0]) == min(cap, n)
        R.assert_same_hillslopes(got, (want[0][:cap], want[1]), f"cap {cap}")
    cnt = C.c_uint32()
    m._chk(m.L.smx_hillslopes(m.h, 3, None, HSZ, 0, C.byref(cnt), *NOPLANES))
    assert cnt.value == n, "cap 0, out NULL: counting only"
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n + 4, 0xFFFFFFFE, np.uint32)
    m._chk(m.L.smx_hillslopes(m.h, 3, capi.ptr(short), 16, n, C.byref(cnt), *NOPLANES))
    assert cnt.value == n and (short[4 * n:] == 0xFFFFFFFE).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["cells"], r["steps_max"], r["farthest_cell"]]
    m.close()


@pytest.mark.parametrize("shape", [(65, 63), (1, 70), (9, 7)], ids=oddmaps.shape_id)
def test_odd_maps(shape):
    s = oddmaps.start("default", shape)
    m = Layermap(oddmaps.cfg_of("default"), shape[0], shape[1], seed=oddmaps.SEED, pool=oddmaps.POOL, initialize=False)
    m.load(s)
    drain = D.drainage(s)
    for t in (1, 3, 8):
        strm = S.streams(s, t, drain)
        got = check(m, s, t, R.hillslopes(s, t, drain, strm), f"odd map {shape} threshold {t}", drain, strm)
        R.assert_same_hillslopes(got, H.run(s, t)[:2], f"odd map {shape} threshold {t}: device against the host-compiled bodies")
    m.close()


# ---------------------------------------------------------------- 2. ticked states
def test_ticked_serial_state_is_the_golden_state():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    got4 = sm.map.hillslopes(4, **ALL)                         # right behind the ticks
    got16 = sm.map.hillslopes(16, **ALL)
    sm.map.sync()
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    drain = D.drainage(s)
    for t, got in ((4, got4), (16, got16)):
        strm = S.streams(s, t, drain)
        R.assert_same_hillslopes(got, R.hillslopes(s, t, drain, strm), f"default64.t20 threshold {t}")
        R.assert_invariants(s, t, got[0], got[1], drain=drain, strm=strm, what=f"default64.t20 threshold {t}")
    # the figures of the restatement (tests/test_hillslopes_host.py GOLDENS)
    assert (len(got4[0]), sum(r["cells"] for r in got4[0]), max(r["steps_max"] for r in got4[0])) == (573, 2235, 3)
    assert (len(got16[0]), sum(r["cells"] for r in got16[0]), max(r["steps_max"] for r in got16[0])) == (114, 2915, 14)
    sm.map.close()


def test_ticked_relaxed_state():
    sm = SoilMachine(cfg64(), dimx=96, dimy=80, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6, sync=True)
    s = sm.map.snapshot()
    drain = D.drainage(s)
    for t in (1, 8, 40):
        strm = S.streams(s, t, drain)
        check(sm.map, s, t, R.hillslopes(s, t, drain, strm), f"relaxed 96x80 threshold {t}", drain, strm)
    sm.map.close()


# ---------------------------------------------------------------- 3. queued work is seen, nothing is changed
def test_hillslopes_see_queued_ticks_and_are_read_only():
    d = DIG["default64"]
    sm = SoilMachine(cfg64(), 64, seed=0, nwater=d["nwater"], nwind=0, dowind=False, pool=1 << 20)
    sm.tick(8, sync=True)
    sm.tick(3)                                               # queued, not waited for
    first = sm.map.hillslopes(8, **ALL)
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters())
    again = sm.map.hillslopes(8, **ALL)
    R.assert_same_hillslopes(first, again, "behind queued ticks against after a sync")
    assert (sm.map.digest(), sm.map.counters()) == before, "hillslopes changed the map or a counter"
    s = sm.map.snapshot()
    R.assert_same_hillslopes(again, R.hillslopes(s, 8), "after 11 ticks")
    sm.map.close()


def test_the_sibling_analyses_are_what_they_were():
    s, drain, strm, want = R.case("random_bernoulli20", (96, 80), 3)
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    d0, l0, s0 = m.drainage(**DRAIN_ALL), m.lakes(labels=True), m.streams(3, **STREAMS_ALL)
    D.assert_same_drainage(d0, drain, "drainage before")
    S.assert_same_streams(s0, strm, "streams before")
    check(m, s, 3, want, "hillslopes, first", drain, strm)
    d1, l1, s1 = m.drainage(**DRAIN_ALL), m.lakes(labels=True), m.streams(3, **STREAMS_ALL)
    c8 = R.case("random_bernoulli20", (96, 80), 8)
    check(m, s, 8, c8[3], "hillslopes, second", drain, c8[2])
    d2, l2, s2 = m.drainage(**DRAIN_ALL), m.lakes(labels=True), m.streams(3, **STREAMS_ALL)
    for tag, d, l, st in (("between", d1, l1, s1), ("after", d2, l2, s2)):
        assert d[0] == d0[0] and all(np.array_equal(d[1][p], d0[1][p]) for p in D.PLANES), f"drainage {tag} the hillslopes calls"
        assert l[0] == l0[0] and np.array_equal(l[1], l0[1]), f"lakes {tag} the hillslopes calls"
        assert st[0] == s0[0] and all(np.array_equal(st[1][p], s0[1][p]) for p in S.PLANES), f"streams {tag} the hillslopes calls"
    lakes_ref.assert_same_census(l2, lakes_ref.census(s), "smx_lakes after the hillslopes calls")
    # record k belongs to segment k of streams() with the same threshold
    assert [r["first_cell"] for r in m.hillslopes(3)] == [g["first_cell"] for g in s2[0]]
    m.close()


def test_a_larger_map_after_a_smaller_one():
    cfg = cfg64()
    with Ensemble(0) as ens:
        small, big = R.case("random_bernoulli20", (33, 47), 8), R.case("random_bernoulli20", (96, 80), 8)
        a = ens.add(cfg, 33, 47, seed=1, pool=POOL, initialize=False)
        a.load(small[0])
        R.assert_same_hillslopes((ens.hillslopes(8)[0], None), small[3], "the small member alone")
        b = ens.add(cfg, 96, 80, seed=1, pool=POOL, initialize=False)
        b.load(big[0])
        got = ens.hillslopes(8)                                # the ensemble's scratch regrows: more cells, more records
        R.assert_same_hillslopes((got[0], None), small[3], "the small member beside the large one")
        R.assert_same_hillslopes((got[1], None), big[3], "the large member")
    for dims in ((33, 47), (128, 128), (64, 64)):              # a context per size, and one context's calls with growing record counts
        s, drain, strm, want = R.case("random_bernoulli20", dims, 8)
        m = Layermap(cfg, dims[0], dims[1], seed=0, pool=POOL, initialize=False)
        m.load(s)
        R.assert_same_hillslopes((m.hillslopes(8, cap=2), None), (want[0][:2], None), f"{dims}: two records")
        check(m, s, 8, want, f"{dims} after a call with two records", drain, strm)
        m.close()


# ---------------------------------------------------------------- 4. an ensemble of mixed dimensions
def test_ensemble_of_mixed_dimensions():
    which = (("random_bernoulli20", (64, 64)), ("spiral", (33, 47)), ("ties", (1, 70)), ("cone", (96, 80)), ("corners", (70, 1)))
    cases = [R.case(nm, dm, 8) for nm, dm in which]
    cfg = cfg64()
    with Ensemble(0) as ens:
        assert ens.hillslopes(8) == []
        assert ens.L.smx_ensemble_hillslopes(ens.h, 8, None, HSZ, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = []
        for c in cases:
            mem.append(ens.add(cfg, int(c[0].dimx), int(c[0].dimy), seed=1, pool=POOL, initialize=False))
            mem[-1].load(c[0])
        got = ens.hillslopes(8)
        counts = [len(x) for x in got]
        for i, (m, (s, drain, strm, want)) in enumerate(zip(mem, cases)):
            own = check(m, s, 8, want, f"member {i} by itself", drain, strm)
            R.assert_same_hillslopes((got[i], None), want, f"member {i} in the ensemble call")
            R.assert_same_hillslopes((got[i], None), own, f"member {i}: the ensemble call against its own")
        assert max(counts) > 3
        # fewer records than a member has segments: the counts stay, the records are cut, in the caller's layout
        cap = 3
        out = (capi.Hillslope * (len(mem) * cap))()
        n = np.zeros(len(mem), np.uint32)
        ens._chk(ens.L.smx_ensemble_hillslopes(ens.h, 8, out, HSZ, cap, capi.ptr(n)))
        assert [int(v) for v in n] == counts
        for i in range(len(mem)):
            k = min(cap, counts[i])
            R.assert_same_hillslopes(([out[i * cap + r].as_dict() for r in range(k)], None), (got[i][:cap], None), f"cap 3, member {i}")
        assert [len(x) for x in ens.hillslopes(8, cap=1)] == [min(1, c) for c in counts]
        for t in (1, 3):                                       # other round counts, the largest member's bound for all
            got = ens.hillslopes(t)
            for i, (nm, dm) in enumerate(which):
                R.assert_same_hillslopes((got[i], None), R.case(nm, dm, t)[3], f"member {i} threshold {t}")


# ---------------------------------------------------------------- 5. errors
def test_refused_arguments():
    L = capi.load()
    n = C.c_uint32(7)
    assert L.smx_hillslopes(None, 3, None, HSZ, 0, C.byref(n), *NOPLANES) == -2 and n.value == 7
    assert L.smx_ensemble_hillslopes(None, 3, None, HSZ, 0, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_hillslopes(strip.h, 3, None, HSZ, 0, C.byref(n), *NOPLANES) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.hillslopes(3)
    strip.close()
    s, drain, strm, want = R.case("random_bernoulli20", (64, 64), 3)
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert L.smx_hillslopes(m.h, 3, None, 0, 0, C.byref(n), *NOPLANES) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_hillslopes(m.h, 0, None, HSZ, 0, C.byref(n), *NOPLANES) == -2 and b"threshold" in L.smx_last_error(m.h)
    assert L.smx_hillslopes(m.h, 3, None, HSZ, 0, None, *NOPLANES) == -2 and b"nsegments is null" in L.smx_last_error(m.h)
    assert L.smx_hillslopes(m.h, 3, None, HSZ, 3, C.byref(n), *NOPLANES) == -2 and b"out is null" in L.smx_last_error(m.h), "records asked for, nowhere to put them"
    assert n.value == 7
    with pytest.raises(SoilmxError, match="threshold"):
        m.hillslopes(0)
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        one = capi.ptr(np.zeros(1, np.uint32))
        assert L.smx_ensemble_hillslopes(ens.h, 3, None, 0, 0, one) == -2 and b"struct_size" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_hillslopes(ens.h, 0, None, HSZ, 0, one) == -2 and b"threshold" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_hillslopes(ens.h, 3, None, HSZ, 0, None) == -2 and b"nsegments is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_hillslopes(ens.h, 3, None, HSZ, 2, one) == -2 and b"out is null" in L.smx_ensemble_last_error(ens.h)
        assert [len(x) for x in ens.hillslopes(1)] == [len(e.hillslopes(1))]
    check(m, s, 3, want, "after the refused calls", drain, strm)
    m.close()                                                # (the hillslope scratch goes with the context)
