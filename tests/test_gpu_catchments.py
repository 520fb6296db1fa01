"""The catchments of listed outlets on a real MI355X (smx_catchments / smx_ensemble_catchments): every record field, the four planes
and the hypsometry tables equal the restatement tests/catchments_ref.py exactly -- doubles by their bits -- and equal the same kernel
bodies compiled for the host (tests/catchments_host)."""
import ctypes as C

import numpy as np
import pytest

import catchments_ref as R
import drainage_ref as D
import flowpaths_ref as F
import hillslopes_ref
import oddmaps
import streams_ref as S
from catchments_host_lib import catchments as H
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare
from test_catchments_host import EDGE, check_hand, check_line

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 17
NONE = R.NONE
ALL = dict(gauge=True, straight=True, diagonal=True, drop=True)
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
CSZ = C.sizeof(capi.Catchment)
NOPLANES = (None,) * 4


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def fetch(m, cells, bins=0, bin_height=None, **planes):
    """m.catchments -> (records, planes or None, hist or None)."""
    got = m.catchments(cells, bins=bins, bin_height=bin_height, **planes)
    recs, pl = got if planes else (got, None)
    return recs, pl, (np.array([r["hist"] for r in recs], np.uint32) if bins else None)


def check(m, s, cells, want, what, bins=0, bin_height=None, drain=None, paths=None):
    """All planes together against `want`, and the invariants on what the device gave."""
    got = fetch(m, cells, bins, bin_height, **ALL)
    R.assert_same_catchments(got, want, what)
    R.assert_invariants(s, cells, *got, drain=drain, paths=paths, what=what)
    assert all(r["drop_sum"] == r["drop_sum_q40"] * 2.0 ** -40 for r in got[0])
    return got


# ---------------------------------------------------------------- 1. the inputs and the lists
@pytest.mark.parametrize("dims", D.SIZES + [D.BIG], ids=lambda d: f"{d[0]}x{d[1]}")
def test_inputs_equal_the_restatement_and_the_host_bodies(dims):
    names = sorted(D.INPUTS) if dims != D.BIG else D.BIG_INPUTS           # (128^2: many tiles and several fold blocks)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in names:
        paths = F.case(name, dims)[2]
        m.load(D.case(name, dims)[0])
        for which in ("lowest", "every7", "every", "sample"):
            bins = {"every7": 7, "sample": 64}.get(which, 0)
            s, drain, cells, want = R.case(name, dims, which, bins, EDGE)
            what = f"{name} {dims} {which}"
            got = check(m, s, cells, want, what, bins, EDGE, drain, paths)
            if which in ("lowest", "sample"):
                host = H.run(s, cells, bins=bins, bin_height=EDGE)
                R.assert_same_catchments(got, host[:3], f"{what}: device against the host-compiled bodies")
                R.assert_same_catchments(fetch(m, cells), want, f"{what}: records only")
                for p in R.PLANES:                                         # each plane alone
                    recs, planes, _ = fetch(m, cells, **{p: True})
                    assert list(planes) == [p]
                    R.assert_same_catchments((recs, planes, None), want, f"{what}: {p} alone")
    m.close()


@pytest.mark.parametrize("name", ["random_bernoulli20", "plateau"])
def test_wet_cells_and_sinks_only(name):
    m = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    s, drain, cells, want = R.case(name, (64, 64), "terminals")
    m.load(s)
    got = check(m, s, cells, want, f"{name} terminals", drain=drain, paths=F.case(name, (64, 64))[2])
    assert not (got[1]["gauge"] == NONE).any() and all(r["downstream"] == NONE and r["flags"] & 6 for r in got[0])
    m.close()


def test_nested_gauges_along_the_spiral():
    for dims in ((64, 64), (96, 80)):                          # twelve and thirteen rounds: the fold reads either set
        m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
        s, drain, cells, want = R.case("spiral", dims, "path100", 7, EDGE)
        m.load(s)
        got = check(m, s, cells, want, f"spiral {dims}", 7, EDGE, drain, F.case("spiral", dims)[2])
        check_line(s, drain, cells, got)
        host = H.run(s, cells, bins=7, bin_height=EDGE)
        R.assert_same_catchments(got, host[:3], f"spiral {dims}: device against the host-compiled bodies")
        m.close()


def test_hand_built_map():
    m = Layermap(cfg64(), 5, 5, seed=0, pool=POOL, initialize=False)
    s, drain, cells, want = R.hand_case()
    m.load(s)
    got = check(m, s, cells, want, "hand-built", 3, 1.0, drain, F.flowpaths(s, drain))
    check_hand(*got)                                           # the numbers tests/test_catchments_host.py writes out by hand
    pairs = m.catchments([(4, 2), (2, 2), (1, 1)])             # the same gauges as (x, y)
    assert not any(R.same(a, b) for a, b in zip(pairs, want[0]))
    m.close()


@pytest.mark.parametrize("bins,bh", [(1, EDGE), (7, EDGE), (64, EDGE), (64, 2.0 ** -12)], ids=["1", "7", "64", "64-tiny"])
def test_hypsometry(bins, bh):
    m = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    s, drain, cells, want = R.case("random_bernoulli20", (64, 64), "sample", bins, bh)
    m.load(s)
    got = check(m, s, cells, want, f"bins {bins} bin_height {bh}", bins, bh, drain)
    assert [int(v) for v in got[2].sum(axis=1)] == [r["cells"] for r in got[0]]
    m.close()


# ---------------------------------------------------------------- 2. odd maps
@pytest.mark.parametrize("shape", [(65, 63), (1, 70), (9, 7)], ids=oddmaps.shape_id)
def test_odd_maps(shape):
    n = shape[0] * shape[1]
    cfg = oddmaps.cfg_of("default")
    dry = Layermap(cfg, shape[0], shape[1], seed=oddmaps.SEED, pool=oddmaps.POOL)          # the initial terrain, dry
    states = [("dry", dry, dry.snapshot())]
    wet = Layermap(cfg, shape[0], shape[1], seed=oddmaps.SEED, pool=oddmaps.POOL, initialize=False)
    wet.load(oddmaps.start("default", shape))
    states.append(("wet start", wet, oddmaps.start("default", shape)))
    for tag, m, s in states:
        drain = D.drainage(s)
        paths = F.flowpaths(s, drain)
        for which in ("lowest", "every7", "terminals"):
            cells = R.LISTS[which](s, drain)
            want = R.catchments(s, cells, 7, 0.125, drain)
            got = check(m, s, cells, want, f"odd map {shape} {tag} {which}", 7, 0.125, drain, paths)
            R.assert_same_catchments(got, H.run(s, cells, bins=7, bin_height=0.125)[:3], f"odd map {shape} {tag} {which}: device against the host-compiled bodies")
        m.close()
    assert n == len(states[0][2].count)


# ---------------------------------------------------------------- 3. ticked states: queued work is seen, nothing is changed
def outlets(m, threshold=8):
    """the last cells of the streams(threshold) segments"""
    return [g["last_cell"] for g in m.streams(threshold)]


def test_ticked_serial_state_is_the_golden_state_and_stays_it():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(17, sync=True)
    sm.tick(3)                                                 # queued, not waited for
    probe = [5, 4000, 2077]
    first = fetch(sm.map, probe, 8, 0.25, **ALL)               # right behind the ticks
    sm.map.sync()
    before = (sm.map.digest(), sm.map.counters())
    cells = outlets(sm.map)
    got = fetch(sm.map, cells, 8, 0.25, **ALL)
    again = fetch(sm.map, probe, 8, 0.25, **ALL)
    assert (sm.map.digest(), sm.map.counters()) == before, "catchments changed the map or a counter"
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    drain = D.drainage(s)
    paths = F.flowpaths(s, drain)
    assert cells == [g["last_cell"] for g in S.streams(s, 8, drain)[0]] and len(set(cells)) == len(cells) > 20
    R.assert_same_catchments(first, R.catchments(s, probe, 8, 0.25, drain), "default64.t20 behind queued ticks")
    R.assert_same_catchments(again, first, "default64.t20 after a sync")
    R.assert_same_catchments(got, R.catchments(s, cells, 8, 0.25, drain), "default64.t20, the outlets of streams(8)")
    R.assert_invariants(s, cells, *got, drain=drain, paths=paths, what="default64.t20")
    segs = S.streams(s, 8, drain)[0]
    assert all(r["area"] == g["area_last"] for r, g in zip(got[0], segs)), "a segment's outlet gauges the segment's area"
    sm.map.close()


def test_ticked_relaxed_state():
    sm = SoilMachine(cfg64(), dimx=64, dimy=64, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6, sync=True)
    before = sm.map.digest()
    cells = outlets(sm.map)
    got = fetch(sm.map, cells, 8, 0.25, **ALL)
    assert sm.map.digest() == before, "catchments changed the map"
    s = sm.map.snapshot()
    drain = D.drainage(s)
    assert cells == [g["last_cell"] for g in S.streams(s, 8, drain)[0]] and len(cells) > 20
    R.assert_same_catchments(got, R.catchments(s, cells, 8, 0.25, drain), "relaxed 64x64, the outlets of streams(8)")
    R.assert_invariants(s, cells, *got, drain=drain, paths=F.flowpaths(s, drain), what="relaxed 64x64")
    sm.map.close()


def test_the_sibling_analyses_are_what_they_were():
    s, drain = D.case("random_bernoulli20", (96, 80))
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    hall = dict(entry=True, hillslope=True, straight=True, diagonal=True, hand=True)
    pall = dict(terminal=True, straight=True, diagonal=True, drop=True, upstream=True, source=True, stem=True)
    sall = dict(order=True, segments=True, reach=True, heads=True)

    def siblings():
        return m.drainage(**DRAIN_ALL), m.streams(3, **sall), m.hillslopes(3, **hall), m.flowpaths(**pall)

    def same(a, b):
        return a[0] == b[0] and sorted(a[1]) == sorted(b[1]) and all(np.array_equal(a[1][p].view(np.uint8), b[1][p].view(np.uint8)) for p in a[1])

    first = siblings()
    D.assert_same_drainage(first[0], drain, "drainage before")
    F.assert_same_flowpaths(first[3], F.case("random_bernoulli20", (96, 80))[2][:2], "flowpaths before")
    hillslopes_ref.assert_same_hillslopes(first[2], hillslopes_ref.case("random_bernoulli20", (96, 80), 3)[3], "hillslopes before")
    for which, bins in (("sample", 64), ("every7", 0)):
        _, _, cells, want = R.case("random_bernoulli20", (96, 80), which, bins, EDGE)
        check(m, s, cells, want, f"catchments, {which}", bins, EDGE, drain)
        assert all(same(a, b) for a, b in zip(siblings(), first)), f"a sibling analysis changed behind catchments({which})"
    m.close()


# ---------------------------------------------------------------- 4. the scratch grows and shrinks with the calls
def test_scratch_growth():
    cfg = cfg64()
    small, big = D.case("random_bernoulli20", (16, 16)), D.case("random_bernoulli20", (128, 128))

    def fresh(s, cells, bins):
        """the same call on a context nobody has used before"""
        m = Layermap(cfg, int(s.dimx), int(s.dimy), seed=0, pool=POOL, initialize=False)
        m.load(s)
        got = fetch(m, cells, bins, EDGE)
        m.close()
        return got[0], got[2]

    def ens_call(ens, cells, bins):
        recs = ens.catchments(cells, bins=bins, bin_height=EDGE if bins else None)
        assert len(recs) == 1
        return recs[0], (np.array([r["hist"] for r in recs[0]], np.uint32) if bins else None)

    rng = np.random.default_rng(17)
    with Ensemble(0) as ens:                                   # one ensemble scratch: 16^2, then 128^2, then 16^2 again
        for s, n, bins in ((small[0], 1, 0), (big[0], 4096, 64), (small[0], 256, 64), (small[0], 1, 0)):
            cells = [int(c) for c in rng.choice(int(s.dimx) * int(s.dimy), n, replace=False)]
            for m in list(ens.members):
                ens.remove(m)
            a = ens.add(cfg, int(s.dimx), int(s.dimy), seed=1, pool=POOL, initialize=False)
            a.load(s)
            got, want = ens_call(ens, cells, bins), fresh(s, cells, bins)
            R.assert_same_catchments((got[0], None, got[1]), (want[0], None, want[1]), f"ensemble scratch: {s.dimx}x{s.dimy}, {n} gauges, {bins} bins")
    m = Layermap(cfg, 128, 128, seed=0, pool=POOL, initialize=False)       # one context scratch: the list and the bins grow, then shrink
    m.load(big[0])
    for n, bins in ((1, 0), (64, 7), (4096, 64), (1, 0), (4096, 1)):
        cells = [int(c) for c in rng.choice(128 * 128, n, replace=False)]
        got, want = fetch(m, cells, bins, EDGE), fresh(big[0], cells, bins)
        R.assert_same_catchments((got[0], None, got[2]), (want[0], None, want[1]), f"context scratch: {n} gauges, {bins} bins")
        if n <= 64:
            R.assert_same_catchments(got, R.catchments(big[0], cells, bins, EDGE, big[1]), f"context scratch: {n} gauges against the restatement")
    m.close()


# ---------------------------------------------------------------- 5. ensembles
def test_ensemble_of_mixed_dimensions():
    which = (("random_bernoulli20", (64, 64)), ("spiral", (33, 47)), ("ties", (1, 70)))
    snaps = [D.case(nm, dm) for nm, dm in which]
    cells = [69, 0, 35, 7, 68, 13]                             # inside the smallest member
    cfg = cfg64()
    with Ensemble(0) as ens:
        assert ens.catchments(cells) == []
        assert ens.L.smx_ensemble_catchments(ens.h, None, 0, None, CSZ, None, 0, 0.0) == 0, "an empty ensemble: 0, nothing written"
        mem = []
        for s, _ in snaps:
            mem.append(ens.add(cfg, int(s.dimx), int(s.dimy), seed=1, pool=POOL, initialize=False))
            mem[-1].load(s)
        got = ens.catchments(cells, bins=7, bin_height=EDGE)
        for i, (m, (s, drain)) in enumerate(zip(mem, snaps)):
            want = R.catchments(s, cells, 7, EDGE, drain)
            own = check(m, s, cells, want, f"member {i} by itself", 7, EDGE, drain)
            mine = (got[i], None, np.array([r["hist"] for r in got[i]], np.uint32))
            R.assert_same_catchments(mine, want, f"member {i} in the ensemble call")
            R.assert_same_catchments(mine, own, f"member {i}: the ensemble call against its own")
        with pytest.raises(SoilmxError, match=r"cells\[1\] is 70, outside member 2"):
            ens.catchments([3, 70])


def test_a_fork_into_eight_members():
    s, drain, cells, want = R.case("random_bernoulli20", (64, 64), "sample", 7, EDGE)
    base = Layermap(cfg64(), 64, 64, seed=0, pool=POOL, initialize=False)
    base.load(s)
    with Ensemble(0) as ens:
        ens.fork(base, 8, seeds=list(range(8)), pool=POOL)
        got = ens.catchments(cells, bins=7, bin_height=EDGE)
        assert len(got) == 8
        for i in range(8):
            R.assert_same_catchments((got[i], None, np.array([r["hist"] for r in got[i]], np.uint32)), want, f"fork member {i}")
    base.close()


# ---------------------------------------------------------------- 6. a short struct, refused arguments
def test_a_short_struct_gives_the_prefix():
    s, drain, cells, want = R.case("cone", (33, 47), "sample")
    m = Layermap(cfg64(), 33, 47, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = len(cells)
    cl = np.array(cells, np.uint32)
    short = np.full(4 * n + 4, 0xFFFFFFFE, np.uint32)
    m._chk(m.L.smx_catchments(m.h, capi.ptr(cl), n, capi.ptr(short), 16, None, 0, 0.0, *NOPLANES))
    assert (short[4 * n:] == 0xFFFFFFFE).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["cell"], r["cells"], r["area"], r["downstream"]]
    m.close()


def test_refused_arguments():
    L = capi.load()
    cfg = cfg64()
    cl = np.array([5, 9, 70], np.uint32)
    assert L.smx_catchments(None, capi.ptr(cl), 3, None, CSZ, None, 0, 0.0, *NOPLANES) == -2
    assert L.smx_ensemble_catchments(None, capi.ptr(cl), 3, None, CSZ, None, 0, 0.0) == -2
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    out = (capi.Catchment * 4)()
    assert L.smx_catchments(strip.h, capi.ptr(cl), 3, out, CSZ, None, 0, 0.0, *NOPLANES) == -2 and b"strip context" in L.smx_last_error(strip.h)
    with pytest.raises(SoilmxError, match="strip"):
        strip.catchments([1])
    strip.close()
    s, drain = D.case("random_bernoulli20", (64, 64))
    m = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    m.load(s)
    dup = np.array([5, 9, 70, 9, 5], np.uint32)
    far = np.array([5, 4096, 70], np.uint32)
    hist = np.full(3 * 64 + 1, 0xCACACACA, np.uint32)
    planes = [np.full(4096, 0xCACACACA, np.uint32) for _ in range(3)] + [np.full(4096, -7.5)]
    pl = [capi.ptr(p) for p in planes]
    h = capi.ptr(hist)
    refused = [
        ((None, 3, out, CSZ, h, 7, 1.0), b"cells is null"),
        ((capi.ptr(cl), 0, out, CSZ, h, 7, 1.0), b"n is 0"),
        ((capi.ptr(cl), 3, None, CSZ, h, 7, 1.0), b"out is null"),
        ((capi.ptr(cl), 3, out, 0, h, 7, 1.0), b"struct_size is 0"),
        ((capi.ptr(far), 3, out, CSZ, h, 7, 1.0), b"cells[1] is 4096, outside the map (4096 cells)"),
        ((capi.ptr(dup), 5, out, CSZ, h, 7, 1.0), b"cells[3] repeats cells[1] (cell 9)"),
        ((capi.ptr(cl), 3, out, CSZ, h, 65, 1.0), b"nbins is 65"),
        ((capi.ptr(cl), 3, out, CSZ, None, 7, 1.0), b"hist is null while nbins is 7"),
        ((capi.ptr(cl), 3, out, CSZ, h, 7, 0.0), b"bin_height is"),
        ((capi.ptr(cl), 3, out, CSZ, h, 7, -1.0), b"bin_height is"),
        ((capi.ptr(cl), 3, out, CSZ, h, 7, float("inf")), b"bin_height is"),
        ((capi.ptr(cl), 3, out, CSZ, h, 7, float("nan")), b"bin_height is"),
        ((capi.ptr(cl), 1 << 25, out, CSZ, h, 64, 1.0), b"n * nbins is 2147483648"),          # (refused for its size: the list is not read)
    ]
    C.memset(out, 0xCA, C.sizeof(out))
    canary = bytes(out)
    for args, text in refused:
        assert L.smx_catchments(m.h, *args, *pl) == -2 and text in L.smx_last_error(m.h), (text, L.smx_last_error(m.h))
        assert bytes(out) == canary and (hist == 0xCACACACA).all() and all((p == 0xCACACACA).all() for p in planes[:3]) and (planes[3] == -7.5).all(), text
    with Ensemble(0) as ens:
        e = ens.add(cfg, 33, 47, seed=1, pool=POOL)
        ens.add(cfg, 9, 7, seed=1, pool=POOL)
        for args, text in refused:
            text = b"cells[1] is 4096, outside member 1 (63 cells)" if text.startswith(b"cells[1] is 4096") else text
            if text.startswith(b"cells[3] repeats"):
                args = (capi.ptr(np.array([5, 9, 7, 9, 5], np.uint32)),) + args[1:]
            assert L.smx_ensemble_catchments(ens.h, *args) == -2 and text in L.smx_ensemble_last_error(ens.h), (text, L.smx_ensemble_last_error(ens.h))
            assert bytes(out) == canary and (hist == 0xCACACACA).all(), text
        assert [r["cell"] for r in ens.catchments([5, 9])[0]] == [r["cell"] for r in e.catchments([5, 9])] == [5, 9]
    with pytest.raises(SoilmxError, match="repeats"):
        m.catchments([(1, 2), (1, 2)])
    want = R.catchments(s, [5, 9, 70], 7, 1.0, drain)
    check(m, s, [5, 9, 70], want, "after the refused calls", 7, 1.0, drain)
    m.close()                                                # (the catchment scratch goes with the context)
