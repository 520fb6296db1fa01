"""The strata readers on a real MI355X (smx_soil_totals / smx_ensemble_soil_totals / smx_soil_thickness / smx_cores): every integer and
every float bit equals the restatement tests/strata_ref.py AND the same kernel bodies compiled for the host (tests/strata_host).
No test here feeds the device a corrupt chain: that is the host bodies' business (tests/test_strata_host.py)."""
import ctypes as C

import numpy as np
import pytest

import strata_host_lib as H
import strata_ref as R
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 18


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def state(m):
    return m.digest(), m.counters()


def check_all(m, s, what, ref_lists=R.TYPE_LISTS):
    """Every call on map m, which holds snapshot s, against the restatement and the host bodies; the map is left as it was."""
    before = state(m)
    hm = H.HostMap(s)
    n = s.ncells
    for nt in (64, 5):
        got = m.soil_totals(nt, other=True)
        R.assert_same_totals(got, R.totals(s, nt), f"{what}: totals of {nt} types against the restatement")
        R.assert_same_totals(got, H.totals(hm, nt), f"{what}: totals of {nt} types against the host bodies")
        assert all(r["volume"] == r["volume_q40"] * 2.0 ** -40 and r["held"] == r["held_q40"] * 2.0 ** -40 for r in got[0])
    for types in R.TYPE_LISTS:
        got = m.soil_thickness(types, cover=True, sections=True)
        want = H.thickness(hm, types)
        for name, g, w in zip(("thickness", "cover", "sections"), got, want):
            assert R.same_bits(g.reshape(len(types), n), w), f"{what} {types}: {name} against the host bodies"
        if types in ref_lists:
            for name, g, w in zip(("thickness", "cover", "sections"), got, R.thickness(s, types)):
                assert R.same_bits(g.reshape(len(types), n), w), f"{what} {types}: {name} against the restatement"
    R.assert_same_cores(m.cores(np.arange(n)), (s.count, s.type, s.size, s.floor, s.sat), f"{what}: the whole map as one list")
    rng = np.random.default_rng(n)
    cells = rng.integers(0, n, size=min(2 * n + 3, 700))
    got = m.cores(cells)
    R.assert_same_cores(got, R.cores(s, cells), f"{what}: a shuffled list with repeats")
    R.assert_same_cores(got, H.cores(hm, cells)[2:], f"{what}: cores against the host bodies")
    assert state(m) == before, f"{what}: a call changed the map, a counter or the generator"


# ---------------------------------------------------------------- 1. the synthetic columns
@pytest.mark.parametrize("dims", [(1, 1), (5, 7), (96, 80), (128, 128)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_synthetic_columns(dims):
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for shift in (range(R.NPATTERNS) if dims == (1, 1) else (0,)):
        s = R.synthetic(dims, shift)
        m.load(s)
        check_all(m, s, f"{dims} shift {shift}", ref_lists=R.TYPE_LISTS if dims != (128, 128) else R.TYPE_LISTS[:1])
    m.close()


def test_null_outputs_and_a_shorter_struct():
    s = R.synthetic((96, 80))
    m = Layermap(cfg64(), 96, 80, seed=0, pool=POOL, initialize=False)
    m.load(s)
    n, types = s.ncells, np.array(R.TYPE_LISTS[1], np.uint32)
    want = R.thickness(s, list(types))
    for mask in range(8):                        # each NULL combination of the outputs
        outs = [np.full((4, n), 7.0) if mask & 1 else None, np.full((4, n), 7.0) if mask & 2 else None, np.full((4, n), 7, np.uint32) if mask & 4 else None]
        m._chk(m.L.smx_soil_thickness(m.h, capi.ptr(types), 4, *[capi.ptr(a) for a in outs]))
        for a, w in zip(outs, want):
            assert a is None or R.same_bits(a, w), f"outputs {mask:03b}"
    # a caller compiled against a 16-byte struct gets that prefix of each record, at its own stride
    rec, _ = R.totals(s, 64)
    short = np.full(2 * 64 + 2, 0xABABABABABABABAB, np.uint64)
    m._chk(m.L.smx_soil_totals(m.h, capi.ptr(short), 16, 64, None))
    assert [int(v) for v in short[:128:2]] == [r["sections"] for r in rec] and [int(v) for v in short[1:128:2]] == [r["cells"] for r in rec]
    assert int(short[128]) == int(short[129]) == 0xABABABABABABABAB, "nothing behind the last short record"
    # cap one short of the total: count and total, the arrays untouched
    cells = np.array([2, 3, 2, 0, 6], np.uint32)
    wc = R.cores(s, cells)
    total = len(wc[1])
    count, tot = np.zeros(5, np.uint32), C.c_uint64()
    arrs = [np.full(total, 77, np.uint32), np.full(total, 77.0), np.full(total, 77.0), np.full(total, 77.0)]
    assert m.L.smx_cores(m.h, capi.ptr(cells), 5, capi.ptr(count), total - 1, C.byref(tot), *[capi.ptr(a) for a in arrs]) == 1
    assert tot.value == total and (count == wc[0]).all() and all((a == 77).all() for a in arrs)
    assert m.L.smx_cores(m.h, capi.ptr(cells), 5, capi.ptr(count), total, C.byref(tot), *[capi.ptr(a) for a in arrs]) == 0
    R.assert_same_cores((count, *arrs), wc, "cap == total")
    tot.value = 9
    assert m.L.smx_cores(m.h, None, 0, None, 0, C.byref(tot), None, None, None, None) == 0 and tot.value == 0, "n == 0"
    m.close()


# ---------------------------------------------------------------- 2. ticked states
ANCHORS = {"default64": (20, {0: (399, 18910634942656), 1: (4096, 2669365980220864)}),
           "rgps64": (10, {1: (4096, 2288628419001724), 2: (60040, 37482512810019), 4: (60757, 90106993902542)})}


@pytest.mark.parametrize("case", sorted(ANCHORS))
def test_ticked_state_is_the_golden_and_its_totals_the_anchors(case):
    soil, seed, dowind, _ = SNAP_CASES[case]
    ticks, anchors = ANCHORS[case]
    d = DIG[case]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    sm.tick(ticks)
    got = sm.map.soil_totals(other=True)         # right behind the ticks, no sync between
    sm.map.sync()
    s = sm.map.snapshot()
    assert not compare(s, golden_snapshot(case, ticks))
    R.assert_same_totals(got, R.totals(s, len(got[0])), f"{case}.t{ticks}")
    assert len(got[0]) == len(sm.cfg.soils)
    for t, (sections, vol) in anchors.items():
        assert (got[0][t]["sections"], got[0][t]["volume_q40"]) == (sections, vol), f"type {t}"
    if case == "rgps64":
        assert all(got[0][t][k] == 0 for t in (0, 3) for k in ("sections", "cells", "top_cells", "volume_q40", "held_q40", "flags"))
        assert int(s.count.max()) == 893, "the deep-column case"
    # cross-checks with what the project already has
    dg = sm.map.digest()
    assert sum(r["sections"] for r in got[0]) + got[1] == dg["nsec"]
    nt = len(got[0])
    th, ns = sm.map.soil_thickness(list(range(min(nt, 8))), sections=True)
    assert nt > 8 or (ns.sum(axis=0).reshape(-1) == s.count).all(), "the sections planes over all types sum to the export's count"
    check_all(sm.map, s, f"{case}.t{ticks}", ref_lists=R.TYPE_LISTS[:2])
    # a transect: the cores of the cells on the line
    cells, *core = sm.map.transect((3, 60), (50, 7))
    assert [(int(c) // 64, int(c) % 64) for c in cells] == Layermap.transect_cells((3, 60), (50, 7))
    R.assert_same_cores(core, R.cores(s, cells), "transect")
    sm.map.close()


def test_relaxed_engine_state():
    sm = SoilMachine(cfg64(), dimx=96, dimy=80, seed=3, nwater=400, nwind=0, dowind=False, pool=1 << 20, engine=capi.ENGINE_RELAXED)
    sm.tick(6)
    got = sm.map.soil_totals(other=True)
    sm.map.sync()
    s = sm.map.snapshot()
    R.assert_same_totals(got, R.totals(s, len(got[0])), "relaxed 96x80")
    check_all(sm.map, s, "relaxed 96x80", ref_lists=R.TYPE_LISTS[:1])
    sm.map.close()


# ---------------------------------------------------------------- 3. ensembles
def test_ensemble_of_unequal_members_and_forks():
    cfgs = [load_cfg("default.soil"), load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")]
    with Ensemble(0) as ens:
        assert ens.soil_totals(8) == []
        assert ens.L.smx_ensemble_soil_totals(ens.h, None, 48, 8, None) == 0, "an empty ensemble: 0, nothing written"
        mem = [ens.add(cfgs[0], 64, 64, seed=4, pool=1 << 18), ens.add(cfgs[1], 48, 80, seed=1, pool=1 << 19), ens.add(cfgs[2], 33, 47, seed=7, pool=1 << 18)]
        ens.tick([120, None, 60], [0, None, 30], n=4)            # member 1 sits the ticks out
        for nt in (8, 3, 64):
            got, other = ens.soil_totals(nt, other=True)         # behind the queued ticks
            for i, m in enumerate(mem):
                R.assert_same_totals((got[i], other[i]), m.soil_totals(nt, other=True), f"member {i}, {nt} types: the ensemble call against its own")
        ens.sync()
        got, other = ens.soil_totals(8, other=True)
        figs = ens.figures()
        for i, m in enumerate(mem):
            s = m.snapshot()
            R.assert_same_totals((got[i], other[i]), R.totals(s, 8), f"member {i} against the restatement")
            assert got[i][0]["top_cells"] == figs[i]["wet_cells"]
            assert sum(r["sections"] for r in got[i]) + other[i] == figs[i]["nsec"]
        # thickness of Air over columns with no buried Air is the water plane
        s0 = mem[0].snapshot()
        air, ns = mem[0].soil_thickness([0], sections=True)
        water = ens.plane_stats("water", members=[0], var=False, minmax=False, nonzero=False)["mean"]
        top_air = np.zeros(s0.ncells, np.uint32)
        end = np.cumsum(s0.count.astype(np.int64))
        top_air[s0.count > 0] = s0.type[end[s0.count > 0] - 1] == 0
        clean = ns.reshape(-1) == top_air
        assert clean.any() and R.same_bits(air.reshape(-1)[clean], water[clean])
        forks = ens.fork(mem[0], 3, pool=1 << 18)
        got = ens.soil_totals(8)
        for k in range(3):
            R.assert_same_totals((got[3 + k], 0), (got[0], 0), f"fork {k}")
        for i, m in enumerate(forks):
            m._chk(m.L.smx_srand(m.h, 100 + i))
        ens.tick(100, 0, dowind=False)
        got, other = ens.soil_totals(8, other=True)
        for i, m in enumerate(ens.members):
            R.assert_same_totals((got[i], other[i]), m.soil_totals(8, other=True), f"member {i} after the forks ticked")


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_context_usable():
    L = capi.load()
    assert L.smx_soil_totals(None, None, 48, 4, None) == -2 and L.smx_ensemble_soil_totals(None, None, 48, 4, None) == -2
    assert L.smx_soil_thickness(None, None, 1, None, None, None) == -2 and L.smx_cores(None, None, 0, None, 0, None, None, None, None, None) == -2
    cfg = cfg64()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    for call in (lambda: strip.soil_totals(4), lambda: strip.soil_thickness([1]), lambda: strip.cores([0])):
        with pytest.raises(SoilmxError, match=r"strip context.*rc=-2"):
            call()
    strip.close()
    s = R.synthetic((5, 7))
    m = Layermap(cfg, 5, 7, seed=0, pool=POOL, initialize=False)
    m.load(s)
    for nt in (0, 65):
        with pytest.raises(SoilmxError, match=rf"ntypes is {nt}.*rc=-2"):
            m.soil_totals(nt)
    with pytest.raises(SoilmxError, match=r"ntypes is 9.*rc=-2"):
        m.soil_thickness(list(range(9)))
    with pytest.raises(SoilmxError, match=r"type 2 is listed twice.*rc=-2"):
        m.soil_thickness([1, 2, 4, 2])
    with pytest.raises(SoilmxError, match=r"cells\[1\] is 35.*rc=-2"):
        m.cores([34, 35])
    out = (capi.SoilTotal * 4)()
    assert L.smx_soil_totals(m.h, None, 48, 4, None) == -2 and L.smx_soil_totals(m.h, out, 0, 4, None) == -2
    assert L.smx_soil_thickness(m.h, None, 1, None, None, None) == -2 and b"types is null" in L.smx_last_error(m.h)
    with Ensemble(0) as ens:
        for nt in (0, 65):
            assert L.smx_ensemble_soil_totals(ens.h, out, 48, nt, None) == -2 and b"ntypes" in L.smx_ensemble_last_error(ens.h)
    check_all(m, s, "after the refused calls")
    m.close()
