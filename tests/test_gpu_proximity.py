"""Proximity on a real MI355X (smx_proximity / smx_ensemble_proximity): every record field, every buffer row and the three planes
equal the plain-loop restatement tests/proximity_ref.py exactly, and equal the same kernel bodies compiled for the host
(tests/prox_host). The restatement takes the minimum over ALL sites per cell, so each comparison also says that the separable
transform and its tie rule lost nothing."""
import ctypes as C

import numpy as np
import pytest

import lakes_ref
import proximity_ref as ref
from common import SNAP_CASES, golden_snapshot, load_cfg
from proximity_host_lib import proximity as H
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilmxError

pytestmark = pytest.mark.gpu
POOL = 1 << 17
ALL = dict(nearest=True, group=True, dist2=True)
PSZ = C.sizeof(capi.Proximity)
WATER = ("all", "checker", "spiral", "bernoulli20")
_dry = {}


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def dry(dims):
    if dims not in _dry:
        _dry[dims] = lakes_ref.make_snapshot(np.zeros(dims, bool))
    return _dry[dims]


def fetch(m, cells=None, bins=0, bin_width=1, cap=None, **planes):
    """m.proximity -> (records, planes or None, nrecords)."""
    got = m.proximity(cells, bins=bins, bin_width=bin_width, cap=cap, **planes)
    recs, pl = got if planes else (got, None)
    count = C.c_uint32()
    cl, n = capi.proximity_cells(cells, m.dimy)
    if cl is None:
        m._chk(m.L.smx_proximity(m.h, None, 0, None, PSZ, 0, C.byref(count), None, 0, 1, None, None, None))
    return recs, pl, n if cl is not None else int(count.value)


# ---------------------------------------------------------------- 1. the inputs
def test_the_hand_worked_map():
    m = Layermap(cfg64(), 5, 5, seed=0, pool=POOL, initialize=False)
    m.load(dry((5, 5)))
    recs, pl, _ = fetch(m, [0, 24], **ALL)
    assert [(r["cells"], r["dist2_max"], r["farthest_cell"], r["dist2_sum"]) for r in recs] == [(15, 16, 4, 100), (10, 9, 9, 40)]
    assert all(pl["group"][i, 4 - i] == 0 for i in range(5)) and pl["group"][2, 2] == 0
    assert fetch(m, [(0, 0), (4, 4)])[0] == recs, "(x, y) pairs name the same cells"
    m.close()


@pytest.mark.parametrize("dims", ref.SIZES, ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(dims):
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    m.load(dry(dims))
    for name in (list(ref.PATTERNS) if dims != (128, 128) else ref.LARGE):
        cl, want = ref.case(name, dims, 5, 3)
        what = f"{name} {dims}"
        if cl is None:                                   # no site: WATER mode on the dry map
            got = fetch(m, None, **ALL)
            assert got[2] == 0 and not got[0] and all((p == ref.NONE).all() for p in got[1].values()), what
            continue
        got = fetch(m, cl, 5, 3, **ALL)
        ref.assert_same_proximity(got, want, what)
        if name in ("mirror", "column_pair", "bernoulli1"):
            ref.assert_same_proximity(got, H.run(dry(dims), cl, bins=5, bin_width=3), f"{what}: device against the host-compiled bodies")
            ref.assert_invariants(dims[0], dims[1], got, cl, fetch_transposed(dims, cl), what)
    m.close()


def fetch_transposed(dims, cl):
    t = Layermap(cfg64(), dims[1], dims[0], seed=0, pool=POOL, initialize=False)
    t.load(dry((dims[1], dims[0])))
    pl = t.proximity(ref.transposed_sites(dims[0], dims[1], cl), nearest=True, dist2=True)[1]
    t.close()
    return pl


@pytest.mark.parametrize("dims", [(64, 64), (33, 47), (1, 70), (70, 1)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_water_mode_on_the_lake_masks(dims):
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in WATER:
        s, want = ref.water_case(name, dims, 4, 2)
        m.load(s)
        got = fetch(m, None, 4, 2, **ALL)
        ref.assert_same_proximity(got, want, f"{name} {dims}")
        lakes = m.lakes()
        assert [(r["site"], r["sites"]) for r in got[0]] == [(k["first_cell"], k["cells"]) for k in lakes], "the records are the lakes of lakes(), in rank order"
    m.close()


def test_all_planes_each_plane_alone_records_only_and_the_bins():
    dims = (96, 80)
    cl, _ = ref.case("bernoulli20", dims)
    m = Layermap(cfg64(), *dims, seed=0, pool=POOL, initialize=False)
    m.load(dry(dims))
    for bins, width in ((0, 1), (1, 1), (64, 1), (1, 3), (64, 3)):
        want = ref.case("bernoulli20", dims, bins, width)[1]
        ref.assert_same_proximity(fetch(m, cl, bins, width, **ALL), want, f"all planes, {bins} bins of {width}")
        ref.assert_same_proximity(fetch(m, cl, bins, width), want, f"records only, {bins} bins of {width}")
    for p in ref.PLANES:
        got = fetch(m, cl, **{p: True})
        assert list(got[1]) == [p]
        ref.assert_same_proximity(got, ref.case("bernoulli20", dims)[1], f"{p} alone")
    m.close()


# ---------------------------------------------------------------- 2. ticked states
@pytest.mark.parametrize("case,tick", [("default64", 20), ("rgps64", 10), ("rocksand48x80", 5)])
def test_golden_snapshots_in_water_mode(case, tick):
    s = golden_snapshot(case, tick)
    dx, dy = int(s.dimx), int(s.dimy)
    m = Layermap(load_cfg(SNAP_CASES[case][0]), dx, dy, seed=0, pool=1 << 20, initialize=False)
    m.load(s)
    before = (m.digest(), m.counters())
    want = ref.proximity(dx, dy, snapshot=s, bins=8, bin_width=2)
    got = fetch(m, None, 8, 2, **ALL)
    ref.assert_same_proximity(got, want, f"{case}.t{tick}")
    ref.assert_same_proximity(got, H.run(s, bins=8, bin_width=2), f"{case}.t{tick}: device against the host-compiled bodies")
    wet = np.flatnonzero(lakes_ref.census(s)[1].reshape(-1) != lakes_ref.DRY)
    ref.assert_invariants(dx, dy, got, wet, None, f"{case}.t{tick}")
    assert (m.digest(), m.counters()) == before, "proximity changed the map or a counter"
    m.close()


def test_a_cap_below_the_lake_count_and_the_counting_call():
    s, want = ref.water_case("bernoulli20", (33, 47), 4, 2)
    assert want[2] > 5
    m = Layermap(cfg64(), 33, 47, seed=0, pool=POOL, initialize=False)
    m.load(s)
    ref.assert_same_proximity(fetch(m, None, 4, 2, cap=5, **ALL), (want[0][:5], want[1], want[2]), "cap 5: the first records, whole planes")
    count = C.c_uint32(0xCACACACA)
    m._chk(m.L.smx_proximity(m.h, None, 0, None, PSZ, 0, C.byref(count), None, 0, 0, None, None, None))
    assert count.value == want[2]
    out = (capi.Proximity * (want[2] + 4))()
    C.memset(out, 0xCA, C.sizeof(out))
    m._chk(m.L.smx_proximity(m.h, None, 0, out, PSZ, want[2] + 4, C.byref(count), None, 0, 0, None, None, None))
    assert count.value == want[2] and all(out[want[2] + k].site == 0xCACACACA for k in range(4)), "nothing behind the last lake"
    short = np.full(3 * want[2] + 3, 0xFFFFFFFE, np.uint32)
    m._chk(m.L.smx_proximity(m.h, None, 0, capi.ptr(short), 12, want[2], C.byref(count), None, 0, 0, None, None, None))
    assert (short[3 * want[2]:] == 0xFFFFFFFE).all() and [int(v) for v in short[:3]] == [want[0][0]["site"], want[0][0]["sites"], want[0][0]["cells"]], "a short struct gives the prefix"
    m.close()


# ---------------------------------------------------------------- 3. ensembles, the scratch, the siblings
def test_an_ensemble_of_three_unequal_maps():
    which = (("bernoulli20", (64, 64)), ("spiral", (33, 47)), ("checker", (1, 70)))
    cl = np.array([69, 3, 40, 0, 17], np.uint32)            # inside the smallest member
    cfg = cfg64()
    with Ensemble(0) as ens:
        assert ens.proximity() == [] and ens.proximity(cl) == []
        assert ens.L.smx_ensemble_proximity(ens.h, None, 5, None, PSZ, 0, None, None, 0, 0) == 0, "an empty ensemble: 0, nothing looked at"
        mem = []
        for name, d in which:
            mem.append(ens.add(cfg, d[0], d[1], seed=1, pool=POOL, initialize=False))
            mem[-1].load(ref.water_case(name, d)[0])
        listed, water = ens.proximity(cl, bins=3, bin_width=2), ens.proximity(bins=4, bin_width=2)
        for i, (m, (name, d)) in enumerate(zip(mem, which)):
            ref.assert_same_proximity((listed[i], None, len(cl)), ref.proximity(d[0], d[1], cl, bins=3, bin_width=2), f"list, member {i} in the ensemble call")
            own = fetch(m, cl, 3, 2)
            ref.assert_same_proximity((listed[i], None, len(cl)), (own[0], None, own[2]), f"list, member {i}: the ensemble call against its own")
            want = ref.water_case(name, d, 4, 2)[1]
            ref.assert_same_proximity((water[i], None, want[2]), want, f"water, member {i} in the ensemble call")
            own = fetch(m, None, 4, 2)
            ref.assert_same_proximity((water[i], None, want[2]), (own[0], None, own[2]), f"water, member {i}: the ensemble call against its own")
        with pytest.raises(SoilmxError, match=r"cells\[0\] is 70, outside member 2"):
            ens.proximity([70])


def test_calls_of_very_different_room_and_the_siblings():
    """One context: 4096 sites, 1 site, water, one after the other; drainage() and lakes() give what they gave before."""
    s, wwant = ref.water_case("bernoulli20", (64, 64), 4, 2)
    m = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    drain, lakes = m.drainage(receivers=True, labels=True, area=True), m.lakes(labels=True)
    before = (m.digest(), m.counters())
    every = np.arange(4096, dtype=np.uint32)[::-1].copy()
    got = fetch(m, every, 2, 1, **ALL)
    assert [r["site"] for r in got[0]] == every.tolist() and all(r["cells"] == 1 and r["buffers"].tolist() == [1, 0] for r in got[0])
    assert np.array_equal(got[1]["nearest"].reshape(-1), np.arange(4096)) and not got[1]["dist2"].any()
    ref.assert_same_proximity(fetch(m, [4095], 5, 3, **ALL), ref.case("last", (64, 64), 5, 3)[1], "one site behind 4096")
    ref.assert_same_proximity(fetch(m, None, 4, 2, **ALL), wwant, "water behind one site")
    ref.assert_same_proximity(fetch(m, [4095], 5, 3, **ALL), ref.case("last", (64, 64), 5, 3)[1], "one site behind water")
    assert (m.digest(), m.counters()) == before, "proximity changed the map or a counter"
    again, lagain = m.drainage(receivers=True, labels=True, area=True), m.lakes(labels=True)
    assert again[0] == drain[0] and all(np.array_equal(again[1][p], drain[1][p]) for p in drain[1]), "drainage changed behind proximity"
    assert lagain[0] == lakes[0] and np.array_equal(lagain[1], lakes[1]), "lakes changed behind proximity"
    m.close()


# ---------------------------------------------------------------- 4. refused arguments
def test_refused_arguments():
    L = capi.load()
    cfg = cfg64()
    out = (capi.Proximity * 8)()
    n1 = C.c_uint32(0xCACACACA)
    assert L.smx_proximity(None, None, 0, out, PSZ, 8, C.byref(n1), None, 0, 0, None, None, None) == -2
    assert L.smx_ensemble_proximity(None, None, 0, out, PSZ, 8, C.byref(n1), None, 0, 0) == -2
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    assert L.smx_proximity(strip.h, None, 0, out, PSZ, 8, C.byref(n1), None, 0, 0, None, None, None) == -2 and b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.proximity()
    strip.close()
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(ref.water_case("bernoulli20", (64, 64))[0])
    counts = np.full(4, 0xCACACACA, np.uint32)
    hist = np.full(8 * 64, 0xCACACACA, np.uint32)
    planes = [np.full(4096, 0xCACACACA, np.uint32) for _ in range(3)]
    pl = [capi.ptr(p) for p in planes]
    c, h = capi.ptr(counts), capi.ptr(hist)
    good = np.array([5, 9, 4095], np.uint32)
    outside = np.array([5, 4096, 7], np.uint32)
    twice = np.array([5, 9, 7, 9], np.uint32)
    g, big = capi.ptr(good), 1 << 26
    refused = [
        ((g, 3, out, 0, 8, c, h, 4, 1), b"struct_size is 0"),
        ((g, 3, out, PSZ, 8, None, h, 4, 1), b"nrecords is null"),
        ((None, 3, out, PSZ, 8, c, h, 4, 1), b"cells is null while n is 3"),
        ((g, 0, out, PSZ, 8, c, h, 4, 1), b"n is 0 while cells is given"),
        ((capi.ptr(outside), 3, out, PSZ, 8, c, h, 4, 1), b"cells[1] is 4096, outside"),
        ((capi.ptr(twice), 4, out, PSZ, 8, c, h, 4, 1), b"cells[3] repeats cells[1] (cell 9)"),
        ((g, 3, out, PSZ, 2, c, h, 4, 1), b"cap is 2 while n is 3"),
        ((g, 3, None, PSZ, 8, c, h, 4, 1), b"out is null while cap is 8"),
        ((None, 0, None, PSZ, 8, c, h, 4, 1), b"out is null while cap is 8"),
        ((g, 3, out, PSZ, 8, c, h, 65, 1), b"nbins is 65"),
        ((g, 3, out, PSZ, 8, c, None, 4, 1), b"hist is null while nbins is 4"),
        ((g, 3, out, PSZ, 8, c, h, 4, 0), b"bin_width is 0 while nbins is 4"),
        ((None, 0, out, PSZ, big, c, h, 32, 1), b"cap * nbins is 2147483648"),
    ]
    C.memset(out, 0xCA, C.sizeof(out))
    canary = bytes(out)

    def untouched():
        return bytes(out) == canary and (counts == 0xCACACACA).all() and (hist == 0xCACACACA).all() and all((p == 0xCACACACA).all() for p in planes)

    for args, text in refused:
        assert L.smx_proximity(m.h, *args, *pl) == -2 and text in L.smx_last_error(m.h), (text, L.smx_last_error(m.h))
        assert untouched(), text
    with Ensemble(0) as ens:
        ens.add(cfg, 64, 64, seed=1, pool=POOL)
        ens.add(cfg, 80, 96, seed=1, pool=POOL)
        for args, text in refused:
            assert L.smx_ensemble_proximity(ens.h, *args) == -2 and text in L.smx_ensemble_last_error(ens.h), (text, L.smx_ensemble_last_error(ens.h))
            assert untouched(), text
        assert [r["site"] for r in ens.proximity([7, 2])[1]] == [7, 2]
    wide = Layermap(cfg, capi.PROXIMITY_MAX_SIDE + 1, 1, seed=0, pool=POOL, initialize=False)
    assert L.smx_proximity(wide.h, g, 3, out, PSZ, 8, c, None, 0, 0, None, None, None) == -2 and b"at most 32768 cells a side" in L.smx_last_error(wide.h)
    assert untouched()
    wide.close()
    with pytest.raises(ValueError, match="cells is empty"):
        m.proximity([])
    with pytest.raises(SoilmxError, match="nbins is 65"):
        m.proximity([1], bins=65)
    ref.assert_same_proximity(fetch(m, [4095], 5, 3, **ALL), ref.case("last", (64, 64), 5, 3)[1], "after the refused calls")
    m.close()                                                # (the proximity scratch goes with the context)
