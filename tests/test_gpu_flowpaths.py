"""The flow paths on a real MI355X (smx_flowpaths / smx_ensemble_flowpaths): every record field, both counts, the seven planes and
the profile equal the restatement tests/flowpaths_ref.py exactly -- doubles by their bits -- and equal the same kernel bodies
compiled for the host (tests/flowpaths_host)."""
import ctypes as C

import numpy as np
import pytest

import drainage_ref as D
from analysis_host_lib import flowpaths as H
import flowpaths_ref as R
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare
from test_flowpaths_host import check_hand

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
ALL = dict(terminal=True, straight=True, diagonal=True, drop=True, upstream=True, source=True, stem=True)
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
FSZ = C.sizeof(capi.Flowpath)
NOPLANES = (None,) * 7
NOPROFILE = (None, 0, None)


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def profile_of(recs, nprofile=None):
    """The one cell list back from the records' slices."""
    p = np.concatenate([r["profile"] for r in recs]) if recs else np.zeros(0, np.uint32)
    assert nprofile is None or len(p) == nprofile
    return p


def fetch(m, **kw):
    """m.flowpaths with all seven planes and the profiles -> (records, planes, profile)."""
    recs, planes = m.flowpaths(profiles=True, **ALL, **kw)
    return recs, planes, profile_of(recs)


def check(m, s, want, what, drain=None):
    got = fetch(m)
    R.assert_same_flowpaths(got, want, what, nprofile=len(got[2]))
    R.assert_invariants(s, *got, drain=drain, what=what)
    assert all(r["length"] == (r["steps_max"] - r["diagonal"]) + r["diagonal"] * 2.0 ** 0.5 for r in got[0])
    return got


# ---------------------------------------------------------------- 1. the inputs
@pytest.mark.parametrize("dims", D.SIZES + [D.BIG], ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(dims):
    names = sorted(D.INPUTS) if dims != D.BIG else D.BIG_INPUTS           # (128^2: many tiles and several fold blocks)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        s, drain, want = R.case(name, dims)
        m.load(s)
        what = f"{name} {dims}"
        got = check(m, s, want, what, drain)
        host = H.run(s)
        R.assert_same_flowpaths(got, host[:3], f"{what}: device against the host-compiled bodies", count=host[3], nprofile=host[4])
        only = m.flowpaths()                                               # records only
        assert len(only) == len(want[0]) and not any(R.same(a, b) for a, b in zip(only, want[0])) and "profile" not in only[0]
        for p in R.PLANES:                                                 # each plane alone
            recs, planes = m.flowpaths(**{p: True})
            assert list(planes) == [p]
            R.assert_same_flowpaths((recs, planes), want, f"{what}: {p} alone")
        recs = m.flowpaths(profiles=True)                                  # the profile alone
        R.assert_same_flowpaths((recs, None, profile_of(recs)), want, f"{what}: the profile alone", nprofile=len(profile_of(recs)))
    m.close()


# ---------------------------------------------------------------- 2. the long path and the empty basins
def test_the_long_path_the_plateau_and_the_ramps():
    m = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    s, drain, want = R.case("spiral", (64, 64))
    m.load(s)
    recs, planes, prof = check(m, s, want, "spiral 64x64", drain)          # twelve rounds
    assert len(recs) == 1 and recs[0]["steps_max"] == 2046 and len(prof) == 2047 and recs[0]["source_cell"] == 0 and R.rounds(64 * 64) == 12
    assert int((planes["stem"] != R.NONE).sum()) == 2047 and int(planes["upstream"].max()) == 2046
    s, drain, want = R.case("plateau", (64, 64))
    m.load(s)
    recs, planes, prof = check(m, s, want, "plateau 64x64", drain)
    assert len(recs) == 4096 == len(prof) and (prof == np.arange(4096)).all() and all(r["steps_max"] == 0 for r in recs) and not planes["stem"].any()
    m.close()
    for dims in ((1, 70), (70, 1)):
        m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
        s, drain, want = R.case("ramp_x", dims)
        m.load(s)
        recs, planes, prof = check(m, s, want, f"ramp_x {dims}", drain)
        assert len(recs) == 1 and recs[0]["steps_max"] == 69 and list(prof) == list(range(69, -1, -1))
        m.close()


# ---------------------------------------------------------------- 3. the hand-built map
def test_hand_built_map():
    m = Layermap(cfg64(), 16, 16, seed=0, pool=POOL, initialize=False)
    s, drain, want = R.hand_case()
    m.load(s)
    got = check(m, s, want, "hand-built", drain)
    check_hand(got[0], got[1], got[2], len(got[0]), len(got[2]))           # the numbers tests/test_flowpaths_host.py writes out by hand
    host = H.run(s)
    R.assert_same_flowpaths(got, host[:3], "hand-built: device against the host-compiled bodies", count=host[3], nprofile=host[4])
    m.close()


# ---------------------------------------------------------------- 4. caps and counting
def test_caps_counting_and_a_short_struct():
    s, drain, want = R.case("random_bernoulli20", (33, 47))
    cells = 33 * 47
    m = Layermap(cfg64(), 33, 47, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n, npr = len(want[0]), len(want[2])
    assert n > 8 and npr > n
    cnt, pcnt = C.c_uint32(), C.c_uint32()
    for cap in (0, 1, n - 1, n, n + 5):
        for pcap in (0, 1, npr - 1, npr, npr + 5):
            out = (capi.Flowpath * max(1, cap))()
            planes = {p: np.zeros(cells, np.float64 if p == "drop" else np.uint32) for p in R.PLANES}
            prof = np.full(pcap + 1, 0xFFFFFFFE, np.uint32)
            m._chk(m.L.smx_flowpaths(m.h, out, FSZ, cap, C.byref(cnt), *[capi.ptr(planes[p]) for p in R.PLANES], capi.ptr(prof), pcap, C.byref(pcnt)))
            k, pk = min(cap, n), min(pcap, npr)
            assert (cnt.value, pcnt.value) == (n, npr) and (prof[pk:] == 0xFFFFFFFE).all(), f"cap {cap} profile_cap {pcap}: nothing behind what was asked for"
            # with cap == 1 the planes and the profile still cover every basin
            R.assert_same_flowpaths(([out[r].as_dict() for r in range(k)], {p: v.reshape(33, 47) for p, v in planes.items()}, prof[:pk]),
                                    (want[0][:k], want[1], want[2]), f"cap {cap} profile_cap {pcap}")
    for cap in (0, 1, n + 5):
        got = fetch(m, cap=cap)
        assert len(got[0]) == min(cap, n)
        R.assert_same_flowpaths((got[0], got[1], None), (want[0][:cap], want[1], None), f"Layermap.flowpaths(cap={cap})")
        assert all(np.array_equal(r["profile"], want[2][r["profile_at"]:r["profile_at"] + r["steps_max"] + 1]) for r in got[0])
    cnt.value = pcnt.value = 0
    m._chk(m.L.smx_flowpaths(m.h, None, FSZ, 0, C.byref(cnt), *NOPLANES, None, 0, C.byref(pcnt)))
    assert (cnt.value, pcnt.value) == (n, npr), "cap 0, out NULL: counting only"
    cnt.value = 0
    m._chk(m.L.smx_flowpaths(m.h, None, FSZ, 0, C.byref(cnt), *NOPLANES, *NOPROFILE))
    assert cnt.value == n, "nprofile NULL: skipped"
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n + 4, 0xFFFFFFFE, np.uint32)
    m._chk(m.L.smx_flowpaths(m.h, capi.ptr(short), 16, n, C.byref(cnt), *NOPLANES, *NOPROFILE))
    assert cnt.value == n and (short[4 * n:] == 0xFFFFFFFE).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["cells"], r["source_cell"], r["terminal_cell"]]
    m.close()


# ---------------------------------------------------------------- 5. ensembles
def test_ensemble_of_mixed_dimensions():
    which = (("random_bernoulli20", (64, 64)), ("spiral", (33, 47)), ("ties", (1, 70)))
    cases = [R.case(nm, dm) for nm, dm in which]
    cfg = cfg64()
    with Ensemble(0) as ens:
        assert ens.flowpaths() == []
        assert ens.L.smx_ensemble_flowpaths(ens.h, None, FSZ, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = []
        for c in cases:
            mem.append(ens.add(cfg, int(c[0].dimx), int(c[0].dimy), seed=1, pool=POOL, initialize=False))
            mem[-1].load(c[0])
        got = ens.flowpaths()                                   # twelve rounds for all: the largest member's
        counts = [len(x) for x in got]
        for i, (m, (s, drain, want)) in enumerate(zip(mem, cases)):
            own = check(m, s, want, f"member {i} by itself", drain)
            R.assert_same_flowpaths((got[i], None), want, f"member {i} in the ensemble call")          # (profile_at counts within the member)
            R.assert_same_flowpaths((got[i], None), own, f"member {i}: the ensemble call against its own")
        assert max(counts) > 3
        cap = 3
        out = (capi.Flowpath * (len(mem) * cap))()
        n = np.zeros(len(mem), np.uint32)
        ens._chk(ens.L.smx_ensemble_flowpaths(ens.h, out, FSZ, cap, capi.ptr(n)))
        assert [int(v) for v in n] == counts
        for i in range(len(mem)):
            k = min(cap, counts[i])
            R.assert_same_flowpaths(([out[i * cap + r].as_dict() for r in range(k)], None), (got[i][:cap], None), f"cap 3, member {i}")
        # a member added after a first call: the scratch regrows, more cells and more rounds
        big = R.case("cone", (96, 80))
        b = ens.add(cfg, 96, 80, seed=1, pool=POOL, initialize=False)
        b.load(big[0])
        got = ens.flowpaths()
        for i, c in enumerate(cases + [big]):
            R.assert_same_flowpaths((got[i], None), c[2], f"member {i} after the ensemble grew")


# ---------------------------------------------------------------- 6. a simulated state; nothing is changed
def test_ticked_state_is_the_golden_state_and_stays_it():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    got = fetch(sm.map)                                        # right behind the ticks
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters(), sm.map.drainage(**DRAIN_ALL))
    again = fetch(sm.map)
    after = (sm.map.digest(), sm.map.counters(), sm.map.drainage(**DRAIN_ALL))
    assert before[:2] == after[:2], "flowpaths changed the map or a counter"
    assert before[2][0] == after[2][0] and all(np.array_equal(before[2][1][p], after[2][1][p]) for p in D.PLANES), "flowpaths changed what drainage() gives"
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    drain = D.drainage(s)
    want = R.flowpaths(s, drain)
    R.assert_same_flowpaths(got, want, "default64.t20 behind queued ticks", nprofile=len(got[2]))
    R.assert_same_flowpaths(again, want, "default64.t20 after a sync", nprofile=len(again[2]))
    R.assert_invariants(s, *again, drain=drain, what="default64.t20")
    assert [r["first_cell"] for r in again[0]] == [b["first_cell"] for b in after[2][0]], "record k is basin k of drainage()"
    sm.map.close()


# ---------------------------------------------------------------- 7. an independent cross-check on the device
@pytest.mark.parametrize("name,dims", [("random_bernoulli20", (96, 80)), ("empty", (33, 47)), ("spiral", (64, 64))], ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_against_hillslopes_without_a_channel_and_drainage(name, dims):
    s, drain, want = R.case(name, dims)
    cells = dims[0] * dims[1]
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    m.load(s)
    recs, planes, prof = fetch(m)
    # no cell has an area of cells + 1: no channel, so a dry cell's entry is its terminal
    hrecs, hp = m.hillslopes(cells + 1, entry=True, straight=True, diagonal=True, hand=True)
    assert hrecs == []
    wet = hp["entry"] == capi.HILL_NONE
    assert np.array_equal(wet.reshape(-1), D.heights(s)[0])
    assert np.array_equal(hp["entry"][~wet], planes["terminal"][~wet]) and (planes["terminal"][wet] == np.flatnonzero(wet.reshape(-1))).all()
    assert np.array_equal(hp["straight"], planes["straight"]) and np.array_equal(hp["diagonal"], planes["diagonal"])
    assert np.array_equal(hp["hand"].view(np.uint64), planes["drop"].view(np.uint64))
    drecs, dp = m.drainage(receivers=True, labels=True)
    recv, label = dp["receivers"].reshape(-1), dp["labels"].reshape(-1)
    up = planes["upstream"].reshape(-1)
    for k, (r, b) in enumerate(zip(recs, drecs)):
        assert (r["first_cell"], r["cells"]) == (b["first_cell"], b["cells"])
        if not b["flags"] & capi.BASIN_LAKE:
            assert up[b["first_cell"]] == r["steps_max"], f"basin {k}: upstream at the sink"
        path = r["profile"]
        assert len(path) == r["steps_max"] + 1 and (recv[path[:-1]] == path[1:]).all() and (label[path] == k).all(), f"basin {k}: consecutive profile cells"
    assert sum(r["steps_max"] + 1 for r in recs) == len(prof)
    m.close()


# ---------------------------------------------------------------- 8. errors
def test_refused_arguments():
    L = capi.load()
    n = C.c_uint32(7)
    assert L.smx_flowpaths(None, None, FSZ, 0, C.byref(n), *NOPLANES, *NOPROFILE) == -2 and n.value == 7
    assert L.smx_ensemble_flowpaths(None, None, FSZ, 0, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_flowpaths(strip.h, None, FSZ, 0, C.byref(n), *NOPLANES, *NOPROFILE) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.flowpaths()
    strip.close()
    s, drain, want = R.case("random_bernoulli20", (64, 64))
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert L.smx_flowpaths(m.h, None, 0, 0, C.byref(n), *NOPLANES, *NOPROFILE) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_flowpaths(m.h, None, FSZ, 0, None, *NOPLANES, *NOPROFILE) == -2 and b"nbasins is null" in L.smx_last_error(m.h)
    assert L.smx_flowpaths(m.h, None, FSZ, 3, C.byref(n), *NOPLANES, *NOPROFILE) == -2 and b"out is null" in L.smx_last_error(m.h), "records asked for, nowhere to put them"
    assert L.smx_flowpaths(m.h, None, FSZ, 0, C.byref(n), *NOPLANES, None, 5, None) == -2 and b"profile is null" in L.smx_last_error(m.h)
    assert n.value == 7
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        one = capi.ptr(np.zeros(1, np.uint32))
        assert L.smx_ensemble_flowpaths(ens.h, None, 0, 0, one) == -2 and b"struct_size" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_flowpaths(ens.h, None, FSZ, 0, None) == -2 and b"nbasins is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_flowpaths(ens.h, None, FSZ, 2, one) == -2 and b"out is null" in L.smx_ensemble_last_error(ens.h)
        assert [len(x) for x in ens.flowpaths()] == [len(e.flowpaths())]
    check(m, s, want, "after the refused calls", drain)
    m.close()                                                # (the flow path scratch goes with the context)
