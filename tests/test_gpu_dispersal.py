"""Dispersed flow on a real MI355X (smx_dispersal / smx_ensemble_dispersal): every record field and the three planes equal the
restatement tests/dispersal_ref.py of the loaded snapshot exactly -- every figure is an integer."""
import ctypes as C

import numpy as np
import pytest

import dispersal_ref as R
import drainage_ref as D
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare
from test_dispersal_host import check_hand

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
ONE = R.ONE
ALL = dict(area=True, donors=True, receivers=True)
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
PATHS_ALL = dict(terminal=True, straight=True, diagonal=True, drop=True, upstream=True, source=True, stem=True)
DSZ = C.sizeof(capi.Dispersal)
NOPLANES = (None,) * 3
NAMES = ("cone", "ramp_x", "ties", "random_bernoulli20", "empty")
SIZES = ((9, 7), (33, 47), (65, 63), (1, 70), (70, 1))
BIG_NAMES = ("cone", "ramp_y", "spiral")


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def check(m, s, want, what, exponent):
    got = m.dispersal(exponent, **ALL)
    R.assert_same_dispersal(got, want, what)
    R.assert_invariants(s, *got, what=what)
    assert all(r["inflow"] == r["inflow_q24"] / ONE and r["peak"] == r["peak_q24"] / ONE and r["leak_in"] == r["leak_in_q24"] / ONE and
               r["leak_out"] == r["leak_out_q24"] / ONE for r in got[0])
    assert got[1]["area"].dtype == np.uint64 and got[1]["area"].shape == (int(s.dimx), int(s.dimy))
    return got


# ---------------------------------------------------------------- 1. the inputs
@pytest.mark.parametrize("dims", SIZES + (D.BIG,), ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement(dims):
    names = NAMES if dims != D.BIG else BIG_NAMES                         # (128^2: many tiles meet and the list needs many rounds)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        m.load(D.case(name, dims)[0])
        for e in R.EXPONENTS:
            s, drain, want = R.case(name, dims, e)
            what = f"{name} {dims} exponent {e}"
            check(m, s, want, what, e)
            rounds, batches = m.dispersal_rounds()
            assert batches >= 1 and rounds <= dims[0] * dims[1], what
            if e == 1:
                only = m.dispersal(e)                                      # records only
                assert len(only) == len(want[0]) and not any(R.same(a, b) for a, b in zip(only, want[0]))
                for p in R.PLANES:                                         # each plane alone
                    recs, planes = m.dispersal(e, **{p: True})
                    assert list(planes) == [p]
                    R.assert_same_dispersal((recs, planes), want, f"{what}: {p} alone")
    m.close()


def test_ramp_on_one_row_and_one_column_is_d8():
    for dims in ((1, 70), (70, 1)):
        m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
        s, drain = D.case("ramp_x", dims)
        m.load(s)
        for e in (0, 1, 4, 16):
            recs, planes = m.dispersal(e, area=True)
            assert np.array_equal(planes["area"], m.drainage(area=True)[1]["area"].astype(np.uint64) * ONE), f"ramp_x {dims} exponent {e}"
        m.close()


# ---------------------------------------------------------------- 2. the hand-built map
@pytest.mark.parametrize("exponent", (0, 1))
def test_hand_built_map(exponent):
    m = Layermap(cfg64(), 16, 16, seed=0, pool=POOL, initialize=False)
    s, drain, want = R.hand_case(exponent)
    m.load(s)
    got = check(m, s, want, "hand-built", exponent)
    check_hand(got[0], got[1], exponent)                                   # the numbers tests/test_dispersal_host.py writes out by hand
    m.close()


# ---------------------------------------------------------------- 3. ensembles
def test_ensemble_of_mixed_dimensions_and_one_that_grows():
    which = (("random_bernoulli20", (9, 7)), ("empty", (33, 47)), ("ties", (1, 70)))
    cfg = cfg64()
    with Ensemble(0) as ens:
        assert ens.dispersal() == []
        assert ens.L.smx_ensemble_dispersal(ens.h, 1, None, DSZ, 0, None) == 0, "an empty ensemble: 0, nothing written"
        mem = []
        for nm, dm in which:
            mem.append(ens.add(cfg, dm[0], dm[1], seed=1, pool=POOL, initialize=False))
            mem[-1].load(D.case(nm, dm)[0])
        for e in R.EXPONENTS:
            cases = [R.case(nm, dm, e) for nm, dm in which]
            got = ens.dispersal(e)
            assert ens.dispersal_rounds()[0] >= 1
            for i, (m, (s, drain, want)) in enumerate(zip(mem, cases)):
                own = check(m, s, want, f"member {i} by itself, exponent {e}", e)
                R.assert_same_dispersal((got[i], None), want, f"member {i} in the ensemble call, exponent {e}")
                R.assert_same_dispersal((got[i], None), own, f"member {i}: the ensemble call against its own")
        counts = [len(x) for x in got]
        assert max(counts) > 3
        cap = 3
        out = (capi.Dispersal * (len(mem) * cap))()
        n = np.zeros(len(mem), np.uint32)
        ens._chk(ens.L.smx_ensemble_dispersal(ens.h, 4, out, DSZ, cap, capi.ptr(n)))
        assert [int(v) for v in n] == counts
        for i in range(len(mem)):
            k = min(cap, counts[i])
            R.assert_same_dispersal(([out[i * cap + r].as_dict() for r in range(k)], None), (got[i][:cap], None), f"cap 3, member {i}")
        # a member added after a first call: the scratch regrows, more cells and more rounds
        big = ("cone", (65, 63))
        b = ens.add(cfg, 65, 63, seed=1, pool=POOL, initialize=False)
        b.load(D.case(*big)[0])
        got = ens.dispersal(1)
        for i, (nm, dm) in enumerate(which + (big,)):
            R.assert_same_dispersal((got[i], None), R.case(nm, dm, 1)[2], f"member {i} after the ensemble grew")


def test_ensemble_of_many_tiny_members():
    """Eight 1 x 20 ramps (and 33 of them): the members together have more working member-launches than a batch has launches and
    fewer cells than that. The call counts launches, not members: it ends with rc 0 and reports at most `cells` rounds."""
    cfg = cfg64()
    s = D.INPUTS["ramp_x"](1, 20)
    for count in (8, 33):
        with Ensemble(0) as ens:
            mem = []
            for _ in range(count):
                mem.append(ens.add(cfg, 1, 20, seed=1, pool=POOL, initialize=False))
                mem[-1].load(s)
            for e in (0, 1):
                want = R.dispersal(s, e)
                out = (capi.Dispersal * count)()
                n = np.zeros(count, np.uint32)
                assert ens.L.smx_ensemble_dispersal(ens.h, e, out, DSZ, 1, capi.ptr(n)) == 0, ens.L.smx_ensemble_last_error(ens.h)
                got = ens.dispersal(e)
                rounds, batches = ens.dispersal_rounds()
                assert 1 <= rounds <= 20 and batches == 1, f"{count} members: {rounds} rounds in {batches} batches"
                own = mem[0].dispersal(e, **ALL)
                R.assert_same_dispersal(own, want, f"a 1 x 20 ramp by itself, exponent {e}")
                assert mem[0].dispersal_rounds()[0] == rounds, "the ensemble needs the rounds of its members, not their sum"
                for i in range(count):
                    R.assert_same_dispersal((got[i], None), want, f"member {i} of {count}, exponent {e}")
                    R.assert_same_dispersal((got[i], None), own, f"member {i} of {count} against its own call")
                    assert int(n[i]) == 1 and not R.same(out[i].as_dict(), want[0][0])


# ---------------------------------------------------------------- 4. caps, counting, repeated calls
def test_caps_counting_a_short_struct_and_two_calls_in_a_row():
    s, drain, want = R.case("random_bernoulli20", (33, 47), 1)
    cells = 33 * 47
    m = Layermap(cfg64(), 33, 47, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = len(want[0])
    assert n > 8
    cnt = C.c_uint32()
    for cap in (0, 1, n - 1, n, n + 5):
        out = (capi.Dispersal * (cap + 1))()
        C.memset(out, 0xEE, C.sizeof(out))
        planes = {p: np.zeros(cells, np.uint64 if p == "area" else np.uint32) for p in R.PLANES}
        m._chk(m.L.smx_dispersal(m.h, 1, out, DSZ, cap, C.byref(cnt), *[capi.ptr(planes[p]) for p in R.PLANES]))
        k = min(cap, n)
        assert cnt.value == n and all(out[j].first_cell == 0xEEEEEEEE for j in range(k, cap + 1)), f"cap {cap}: nothing behind what was asked for"
        # with cap == 1 the planes still cover every basin
        R.assert_same_dispersal(([out[r].as_dict() for r in range(k)], {p: v.reshape(33, 47) for p, v in planes.items()}), (want[0][:k], want[1]), f"cap {cap}")
    for cap in (0, 1, n + 5):
        got = m.dispersal(1, cap=cap, **ALL)
        R.assert_same_dispersal(got, (want[0][:cap], want[1]), f"Layermap.dispersal(cap={cap})")
    cnt.value = 0
    m._chk(m.L.smx_dispersal(m.h, 1, None, DSZ, 0, C.byref(cnt), *NOPLANES))
    assert cnt.value == n, "cap 0, out NULL: counting only"
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    short = np.full(4 * n + 4, 0xFFFFFFFE, np.uint32)
    m._chk(m.L.smx_dispersal(m.h, 1, capi.ptr(short), 16, n, C.byref(cnt), *NOPLANES))
    assert cnt.value == n and (short[4 * n:] == 0xFFFFFFFE).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["cells"], r["flags"], r["peak_cell"]]
    # two calls in a row are identical, and the rounds are reported
    a, b = m.dispersal(4, **ALL), m.dispersal(4, **ALL)
    assert a[0] == b[0] and all(np.array_equal(a[1][p], b[1][p]) for p in R.PLANES)
    rounds, batches = m.dispersal_rounds()
    assert rounds >= 1 and batches >= 1
    R.assert_same_dispersal(a, R.case("random_bernoulli20", (33, 47), 4)[2], "exponent 4 behind exponent 1")
    m.close()


# ---------------------------------------------------------------- 5. a simulated state; nothing is changed
def test_ticked_state_is_the_golden_state_and_stays_it():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(20)
    got = sm.map.dispersal(1, **ALL)                           # right behind the ticks
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters(), sm.map.drainage(**DRAIN_ALL), sm.map.flowpaths(**PATHS_ALL))
    again = sm.map.dispersal(1, **ALL)
    four = sm.map.dispersal(4, **ALL)
    after = (sm.map.digest(), sm.map.counters(), sm.map.drainage(**DRAIN_ALL), sm.map.flowpaths(**PATHS_ALL))
    assert before[:2] == after[:2], "dispersal changed the map or a counter"
    assert before[2][0] == after[2][0] and all(np.array_equal(before[2][1][p], after[2][1][p]) for p in D.PLANES), "dispersal changed what drainage() gives"
    assert str(before[3][0]) == str(after[3][0]) and all(np.array_equal(before[3][1][p].view(np.uint8), after[3][1][p].view(np.uint8)) for p in PATHS_ALL), \
        "dispersal changed what flowpaths() gives"
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    drain = D.drainage(s)
    want = R.dispersal(s, 1, drain)
    R.assert_same_dispersal(got, want, "default64.t20 behind queued ticks")
    R.assert_same_dispersal(again, want, "default64.t20 after a sync")
    R.assert_same_dispersal(four, R.dispersal(s, 4, drain), "default64.t20 exponent 4")
    R.assert_invariants(s, *again, what="default64.t20")
    assert [(r["first_cell"], r["cells"], r["flags"]) for r in again[0]] == [(b["first_cell"], b["cells"], b["flags"]) for b in after[2][0]], "record k is basin k of drainage()"
    sm.map.close()


# ---------------------------------------------------------------- 6. errors
def test_refused_arguments():
    L = capi.load()
    n = C.c_uint32(7)
    assert L.smx_dispersal(None, 1, None, DSZ, 0, C.byref(n), *NOPLANES) == -2 and n.value == 7
    assert L.smx_ensemble_dispersal(None, 1, None, DSZ, 0, None) == -2
    assert L.smx_get_dispersal_rounds(None, None, None) == -2 and L.smx_ensemble_get_dispersal_rounds(None, None, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_dispersal(strip.h, 1, None, DSZ, 0, C.byref(n), *NOPLANES) == -2
    assert b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.dispersal()
    strip.close()
    s, drain, want = R.case("random_bernoulli20", (33, 47), 1)
    m = Layermap(cfg, 33, 47, seed=0, pool=POOL, initialize=False)
    m.load(s)
    assert L.smx_dispersal(m.h, 1, None, 0, 0, C.byref(n), *NOPLANES) == -2 and b"struct_size" in L.smx_last_error(m.h)
    assert L.smx_dispersal(m.h, 1, None, DSZ, 0, None, *NOPLANES) == -2 and b"nbasins is null" in L.smx_last_error(m.h)
    assert L.smx_dispersal(m.h, 1, None, DSZ, 3, C.byref(n), *NOPLANES) == -2 and b"out is null" in L.smx_last_error(m.h), "records asked for, nowhere to put them"
    assert L.smx_dispersal(m.h, 17, None, DSZ, 0, C.byref(n), *NOPLANES) == -2 and b"exponent is 17" in L.smx_last_error(m.h)
    assert L.smx_dispersal(m.h, 16, None, DSZ, 0, C.byref(n), *NOPLANES) == 0 and n.value == len(want[0])
    n.value = 7
    with pytest.raises(SoilmxError, match="exponent"):
        m.dispersal(17)
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        one = capi.ptr(np.zeros(1, np.uint32))
        assert L.smx_ensemble_dispersal(ens.h, 1, None, 0, 0, one) == -2 and b"struct_size" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_dispersal(ens.h, 1, None, DSZ, 0, None) == -2 and b"nbasins is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_dispersal(ens.h, 1, None, DSZ, 2, one) == -2 and b"out is null" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_dispersal(ens.h, 17, None, DSZ, 0, one) == -2 and b"exponent is 17" in L.smx_ensemble_last_error(ens.h)
        assert [len(x) for x in ens.dispersal()] == [len(e.dispersal())]
    check(m, s, want, "after the refused calls", 1)
    m.close()                                                # (the dispersal scratch goes with the context)
