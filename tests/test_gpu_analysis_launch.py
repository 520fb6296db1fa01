"""The strided launches of the terrain analyses and the strata readers on a real MI355X, at small maps (smx_set_analysis_launch).

Three families of launches are capped, and their workgroups stride over the rest of the work: k_disp_flow (1024 workgroups),
k_spill_relax / k_through_hops / k_through_exit (2048) and the strata readers (8192). At the default caps the second iteration of a
stride starts above half a million cells, where no restatement can follow; the setter brings the caps down to where one can. Every
case here asserts FROM THE RESTATEMENT that its cap forces a second iteration, runs the call, asserts from the getter that the
launch really had `cap` workgroups, and compares with the plain-Python restatement of the loaded snapshot (dispersal_ref, spill_ref,
through_ref, strata_ref): integers exactly, doubles by their bits. No comparison here has a tolerance. The sweeps and rounds may
differ from the uncapped call's (a sweep works in place, a walk carries on): they are held to the bounds test_gpu_spill.py,
test_gpu_through.py and test_gpu_dispersal.py state."""
import ctypes as C

import numpy as np
import pytest

import budget_ref
import catchments_ref
import dispersal_ref as DR
import drainage_ref as D
import flowpaths_ref
import hillslopes_ref
import lakes_ref
import spill_ref as SR
import strata_ref as ST
import streams_ref
import through_ref as TR
from analysis_host_lib import spill as SH
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 18
LANES, STRATA_LANES = 256, 64                       # LAKE_LANES, STRATA_LANES: the work of one workgroup in one iteration
DEFAULTS = {"flow_blocks": 1024, "relax_blocks": 2048, "strata_blocks": 8192}
G = SH.batch()                                      # SPILL_BATCH: the sweeps of one batch
DISP_ALL = dict(area=True, donors=True, receivers=True)
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
RB = "random_bernoulli20"


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def blocks(items, lanes=LANES):
    return -(-items // lanes)


def bound(rounds):
    return -(-rounds // G) * G


def in_force(owner):
    a = owner.analysis_launch()
    return a["flow_blocks"], a["relax_blocks"], a["strata_blocks"]


def new_map(dims, s=None, pool=POOL):
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=pool, initialize=False)
    if s is not None:
        m.load(s)
    return m


def round0(want):
    """The flow's first ready list by the restatement: the givers nobody gives to."""
    return int(((want[1]["donors"] == 0) & (want[1]["receivers"] > 0)).sum())


# ---------------------------------------------------------------- 1. the flow rounds of the dispersal
FLOW_DIMS = (128, 128)                              # (round 0 lists 1873 cells; at 65 x 63 it lists 478: too few for a cap of 2 and more)
_flow = {}


@pytest.fixture(scope="module")
def flow_map():
    _flow["m"] = new_map(FLOW_DIMS, D.case(RB, FLOW_DIMS)[0])
    yield _flow["m"]
    _flow.pop("m").close()


def check_dispersal(m, s, want, e, what, cap, uncapped):
    got = m.dispersal(e, **DISP_ALL)
    grid = m.analysis_launch()["flow_grid"]
    rounds, batches = m.dispersal_rounds()
    DR.assert_same_dispersal(got, want, what)
    assert grid == (cap or uncapped), f"{what}: k_disp_flow had {grid} workgroups"
    assert batches >= 1 and 1 <= rounds <= int(s.dimx) * int(s.dimy), f"{what}: {rounds} rounds in {batches} batches"
    return got


@pytest.mark.parametrize("cap", (1, 2, 3, 7))
def test_flow_strides_over_the_ready_list(flow_map, cap):
    m = flow_map
    cells = FLOW_DIMS[0] * FLOW_DIMS[1]
    for e in DR.EXPONENTS:
        s, drain, want = DR.case(RB, FLOW_DIMS, e)
        n0 = round0(want)
        assert n0 > cap * LANES, f"a wrong case: round 0 lists {n0} cells, {cap} workgroups take them in one iteration"
        assert cap != 7 or n0 < 2 * cap * LANES, "cap 7: a partial second iteration"
        what = f"{RB} {FLOW_DIMS} exponent {e} flow_blocks {cap}"
        m.set_analysis_launch(flow_blocks=cap)
        got = check_dispersal(m, s, want, e, what, cap, blocks(cells))
        DR.assert_invariants(s, *got, what=what)
        if cap == 1 and e == 1:
            only = m.dispersal(e)                                          # records only
            DR.assert_same_dispersal((only, None), want, f"{what}: records only")
            for p in DR.PLANES:                                            # each plane alone
                recs, planes = m.dispersal(e, **{p: True})
                assert list(planes) == [p]
                DR.assert_same_dispersal((recs, planes), want, f"{what}: {p} alone")
            assert m.analysis_launch()["flow_grid"] == 1
        m.set_analysis_launch()
        check_dispersal(m, s, want, e, f"{what}, then the default", 0, blocks(cells))


# ---------------------------------------------------------------- 2. the relax sweeps, the hop sweeps and the exit
# spiral is one basin: its boundary list is the map's border, 252 cells, and no cap makes a workgroup take a second iteration. It
# stays at cap 1 as the map on which the cap cuts the grid (16 -> 1) and one partial iteration covers the list; the stride condition
# is asserted for the two other maps at every cap.
RELAX_CASES = [(RB, (33, 47), cap) for cap in (1, 2, 3, 5)] + [("empty", (33, 47), cap) for cap in (1, 2, 3, 5)] + [("spiral", (65, 63), 1)]
NO_STRIDE = {("spiral", (65, 63))}
_relax = {}


@pytest.fixture(scope="module")
def relax_maps():
    yield _relax
    for m in _relax.values():
        m.close()
    _relax.clear()


def check_spill(m, name, s, want, what, cap, uncapped):
    recs, filled = m.spill(filled=True)
    grid = m.analysis_launch()["relax_grid"]
    sweeps, batches = m.spill_sweeps()
    SR.assert_same_spill((recs, filled), want, what)
    assert grid == (cap or uncapped), f"{what}: k_spill_relax had {grid} workgroups"
    assert batches >= 1 and sweeps == batches * G and 0 < sweeps <= bound(want[2]["rounds"]), f"{what}: {sweeps} sweeps in {batches} batches, {want[2]['rounds']} Jacobi rounds"
    return recs, filled


def check_through(m, s, want, what, cap, uncapped):
    recs, planes = m.through(area=True, outlets=True)
    grid = m.analysis_launch()["relax_grid"]
    lsw, hsw, batches = m.through_sweeps()
    TR.assert_same_through((recs, planes), want, what)
    assert grid == (cap or uncapped), f"{what}: k_spill_relax, k_through_hops and k_through_exit had {grid} workgroups"
    assert batches >= 1 and lsw % G == 0 and hsw % G == 0 and lsw + hsw == batches * G, f"{what}: {lsw} + {hsw} sweeps in {batches} batches"
    assert 0 < lsw <= bound(want[2]["level_rounds"]), f"{what}: {lsw} level sweeps, {want[2]['level_rounds']} Jacobi rounds"
    assert 0 < hsw <= bound(want[2]["hop_rounds"]), f"{what}: {hsw} hop sweeps, {want[2]['hop_rounds']} Jacobi rounds"
    return recs, planes


@pytest.mark.parametrize("name,dims,cap", RELAX_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"cap{v}")
def test_relax_hops_and_exit_stride_over_the_boundary_list(relax_maps, name, dims, cap):
    if dims not in relax_maps:
        relax_maps[dims] = new_map(dims)
    m = relax_maps[dims]
    s, base, sp, want = TR.case(name, dims)
    boundary = sp[2]["boundary"]                                          # cells with a pass into another basin or off the map
    if (name, dims) in NO_STRIDE:
        assert cap == 1 and boundary <= LANES < dims[0] * dims[1], "the one-basin map: a part of one workgroup, of a grid the cap cuts"
    else:
        assert boundary > cap * LANES, f"a wrong case: {boundary} boundary cells, {cap} workgroups take them in one iteration"
    m.load(s)
    what = f"{name} {dims} relax_blocks {cap}"
    uncapped = blocks(dims[0] * dims[1])
    m.set_analysis_launch(relax_blocks=cap)
    recs, filled = check_spill(m, name, s, sp, f"spill, {what}", cap, uncapped)
    SR.assert_invariants(name, recs, m.drainage(), f"spill, {what}")
    trecs, planes = check_through(m, s, want, f"through, {what}", cap, uncapped)
    TR.assert_invariants(s, trecs, planes, m.drainage(labels=True, area=True), recs, f"through, {what}")
    m.set_analysis_launch()
    check_spill(m, name, s, sp, f"spill, {what}, then the default", 0, uncapped)
    check_through(m, s, want, f"through, {what}, then the default", 0, uncapped)


# ---------------------------------------------------------------- 3. the strata readers
STRATA_DIMS = (33, 47)                              # 1551 columns, 64 to a workgroup and iteration
SHIFT = {1: 0, 2: 3, 3: 0}                          # the synthetic columns moved so that a 300-section column lies where the test wants one


@pytest.mark.parametrize("cap", (1, 2, 3))
def test_strata_readers_stride_over_the_columns_and_the_list(cap):
    s = ST.synthetic(STRATA_DIMS, SHIFT[cap])
    n = s.ncells
    deep = np.flatnonzero(s.count == ST.DEEP)
    assert n > cap * STRATA_LANES, "a wrong case: one iteration takes every column"
    lo = cap * STRATA_LANES + (cap - 1) * STRATA_LANES                   # the last workgroup's second iteration: [lo, lo + 64)
    assert ((deep >= lo) & (deep < lo + STRATA_LANES)).any(), f"a wrong case: no deep column in cells {lo}..{lo + STRATA_LANES - 1}"
    m = new_map(STRATA_DIMS, s)
    before = m.digest(), m.counters()
    for blocks_set in (cap, 0):
        m.set_analysis_launch(strata_blocks=blocks_set)
        what = f"{STRATA_DIMS} strata_blocks {blocks_set}"
        full = blocks(n, STRATA_LANES)

        def grid_is(want_grid, call):
            got = m.analysis_launch()["strata_grid"]
            assert got == want_grid, f"{what}: {call} had {got} workgroups, expected {want_grid}"

        for nt in (64, 5):
            ST.assert_same_totals(m.soil_totals(nt, other=True), ST.totals(s, nt), f"{what}: totals of {nt} types")
            grid_is(blocks_set or full, "k_strata_totals")
        for types in (ST.TYPE_LISTS[0], ST.EIGHT):                        # one type and eight
            got = m.soil_thickness(types, cover=True, sections=True)
            grid_is(blocks_set or full, "k_strata_thickness")
            for pname, g, w in zip(("thickness", "cover", "sections"), got, ST.thickness(s, types)):
                assert ST.same_bits(g.reshape(len(types), n), w), f"{what} {types}: {pname}"
        # 200 listed cells, repeats among them; deep columns at list positions of a second iteration at every cap here
        cells = np.random.default_rng(200 + cap).integers(0, n, size=200).astype(np.uint32)
        for pos in (100, 196):
            cells[pos] = deep[pos % len(deep)]
        assert len(cells) > cap * STRATA_LANES and (196 // STRATA_LANES) // cap >= 1, "a wrong case: list position 196 is in nobody's second or later iteration"
        ST.assert_same_cores(m.cores(cells), ST.cores(s, cells), f"{what}: 200 listed cells")
        grid_is(blocks_set or blocks(200, STRATA_LANES), "k_core_count and k_core_scatter")
        # a transect: at most 47 cells, a part of one workgroup whatever the cap
        tc, *core = m.transect((2, 45), (31, 3))
        assert [(int(c) // 47, int(c) % 47) for c in tc] == Layermap.transect_cells((2, 45), (31, 3)) and len(tc) <= STRATA_LANES
        ST.assert_same_cores(core, ST.cores(s, tc), f"{what}: the transect")
        grid_is(1, "the transect's k_core_count")
    assert (m.digest(), m.counters()) == before, "a call changed the map or a counter"
    m.close()


def test_ensemble_soil_totals_of_three_unequal_members_at_one_workgroup_each():
    dims = ((33, 47), (5, 7), (9, 7))
    snaps = [ST.synthetic(d, k) for k, d in enumerate(dims)]
    assert snaps[0].ncells > STRATA_LANES >= snaps[1].ncells, "the largest member strides, the smallest is a part of one workgroup"
    cfg = cfg64()
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, d[0], d[1], seed=1, pool=POOL, initialize=False) for d in dims]
        for m, s in zip(mem, snaps):
            m.load(s)
        # (1 // 3 workgroups is none: every member gets one; 3 gives every member one as well; 7 two)
        for blocks_set, grid in ((1, 1), (3, 1), (7, 2), (0, blocks(snaps[0].ncells, STRATA_LANES))):
            ens.set_analysis_launch(strata_blocks=blocks_set)
            for nt in (64, 5):
                got, other = ens.soil_totals(nt, other=True)
                assert ens.analysis_launch()["strata_grid"] == grid, f"strata_blocks {blocks_set}"
                for i, s in enumerate(snaps):
                    ST.assert_same_totals((got[i], other[i]), ST.totals(s, nt), f"member {i}, {nt} types, strata_blocks {blocks_set}")
        assert mem[0].analysis_launch()["strata_grid"] == 0, "the ensemble's call is not the member's"


# ---------------------------------------------------------------- 4. ensembles: one member strides, another fills a part of one workgroup
def test_ensemble_of_mixed_dimensions_with_one_workgroup_a_member():
    which = ((RB, (65, 63)), ("empty", (33, 47)), ("ties", (1, 70)))
    late = ("cone", (65, 63))
    cfg = cfg64()
    cases = [TR.case(nm, dm) for nm, dm in which]
    disp = [DR.case(nm, dm, 1) for nm, dm in which]
    assert round0(disp[0][2]) > LANES > round0(disp[2][2]) and cases[0][2][2]["boundary"] > LANES > cases[2][2][2]["boundary"], \
        "a wrong case: member 0 strides, member 2's lists fill a part of one workgroup"
    with Ensemble(0) as ens:
        mem = []
        for (nm, dm), c in zip(which, cases):
            mem.append(ens.add(cfg, dm[0], dm[1], seed=1, pool=POOL, initialize=False))
            mem[-1].load(c[0])
        ens.set_analysis_launch(flow_blocks=1, relax_blocks=1)
        assert in_force(ens) == (1, 1, DEFAULTS["strata_blocks"])

        def run(names, tag):
            cs = [TR.case(nm, dm) for nm, dm in names]
            ds = [DR.case(nm, dm, 1) for nm, dm in names]
            got = ens.dispersal(1)
            rounds, batches = ens.dispersal_rounds()
            assert ens.analysis_launch()["flow_grid"] == 1 and batches >= 1 and 1 <= rounds <= max(dm[0] * dm[1] for _, dm in names), tag
            sgot = ens.spill()
            sweeps, sb = ens.spill_sweeps()
            assert ens.analysis_launch()["relax_grid"] == 1, tag
            assert sb >= 1 and sweeps == sb * G and 0 < sweeps <= bound(max(c[2][2]["rounds"] for c in cs)), f"{tag}: {sweeps} spill sweeps"
            tgot = ens.through()
            lsw, hsw, tb = ens.through_sweeps()
            assert ens.analysis_launch()["relax_grid"] == 1, tag
            assert tb >= 1 and lsw + hsw == tb * G and 0 < lsw <= bound(max(c[3][2]["level_rounds"] for c in cs)) and 0 < hsw <= bound(max(c[3][2]["hop_rounds"] for c in cs)), \
                f"{tag}: {lsw} + {hsw} through sweeps"
            for i, (m, c, d) in enumerate(zip(mem, cs, ds)):
                what = f"{tag}, member {i}"
                DR.assert_same_dispersal((got[i], None), d[2], f"{what}: dispersal in the ensemble call")
                SR.assert_same_spill((sgot[i], None), c[2], f"{what}: spill in the ensemble call")
                TR.assert_same_through((tgot[i], None), c[3], f"{what}: through in the ensemble call")
                # the member's own calls run at the member's own, default, launch shape
                assert in_force(m) == tuple(DEFAULTS.values())
                cells = int(m.dimx) * int(m.dimy)
                own = check_dispersal(m, c[0], d[2], 1, f"{what} by itself", 0, blocks(cells))
                DR.assert_same_dispersal((got[i], None), own, f"{what}: the ensemble's dispersal against its own")
                srecs, _ = check_spill(m, names[i][0], c[0], c[2], f"{what} by itself", 0, blocks(cells))
                SR.assert_same_spill((sgot[i], None), (srecs, None), f"{what}: the ensemble's spill against its own")
                trecs, _ = check_through(m, c[0], c[3], f"{what} by itself", 0, blocks(cells))
                TR.assert_same_through((tgot[i], None), (trecs, None), f"{what}: the ensemble's through against its own")

        run(which, "three members")
        # a member added after the first calls: the scratch regrows, the launch shape stays the ensemble's
        mem.append(ens.add(cfg, late[1][0], late[1][1], seed=1, pool=POOL, initialize=False))
        mem[-1].load(D.case(*late)[0])
        run(which + (late,), "after the ensemble grew")
        ens.set_analysis_launch()
        full = max(blocks(dm[0] * dm[1]) for _, dm in which + (late,))
        DR.assert_same_dispersal((ens.dispersal(1)[0], None), disp[0][2], "back at the default")
        SR.assert_same_spill((ens.spill()[0], None), cases[0][2], "back at the default")
        assert (ens.analysis_launch()["flow_grid"], ens.analysis_launch()["relax_grid"]) == (full, full)


# ---------------------------------------------------------------- 5. a simulated state
def test_ticked_state_with_every_cap_at_one():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    m = sm.map
    sm.tick(20)
    m.sync()
    s = m.snapshot()
    assert not compare(s, golden_snapshot("default64", 20))
    before = m.digest(), m.counters()
    drain = D.drainage(s)
    sp = SR.spill(s, drain)
    th = TR.through(s, drain, sp)
    # The boundary list (1237 cells) and the columns (4096) stride at one workgroup. The flow's round 0 lists 53 givers on this state:
    # there the cap cuts the grid from 16 workgroups to one, which takes the list in a part of one iteration -- the flow's stride
    # is test_flow_strides_over_the_ready_list's.
    assert sp[2]["boundary"] > LANES and s.ncells > STRATA_LANES
    m.set_analysis_launch(1, 1, 1)
    for e in (1, 4):
        got = check_dispersal(m, s, DR.dispersal(s, e, drain), e, f"default64.t20 exponent {e}", 1, 16)
        DR.assert_invariants(s, *got, what=f"default64.t20 exponent {e}")
    recs, _ = check_spill(m, "default64.t20", s, sp, "default64.t20 spill", 1, 16)
    SR.assert_invariants("default64.t20", recs, m.drainage(), "default64.t20")
    trecs, planes = check_through(m, s, th, "default64.t20 through", 1, 16)
    TR.assert_invariants(s, trecs, planes, m.drainage(labels=True, area=True), recs, "default64.t20")
    nt = len(sm.cfg.soils)
    ST.assert_same_totals(m.soil_totals(other=True), ST.totals(s, nt), "default64.t20 totals")
    assert m.analysis_launch()["strata_grid"] == 1
    types = list(range(min(nt, 8)))
    for pname, g, w in zip(("thickness", "cover", "sections"), m.soil_thickness(types, cover=True, sections=True), ST.thickness(s, types)):
        assert ST.same_bits(g.reshape(len(types), s.ncells), w), f"default64.t20 {pname}"
    assert m.analysis_launch()["strata_grid"] == 1
    assert (m.digest(), m.counters()) == before, "a capped call changed the map or a counter"
    m.close()


# ---------------------------------------------------------------- 6. refusals, and whose the values are
def test_refused_values_change_nothing():
    L = capi.load()
    b, g = (C.c_int32 * 3)(7, 7, 7), (C.c_uint32 * 3)(7, 7, 7)
    assert L.smx_set_analysis_launch(None, 1, 1, 1) == -2 and L.smx_ensemble_set_analysis_launch(None, 1, 1, 1) == -2
    assert L.smx_get_analysis_launch(None, b, g) == -2 and L.smx_ensemble_get_analysis_launch(None, b, g) == -2
    assert list(b) == [7, 7, 7] and list(g) == [7, 7, 7]
    m = new_map((9, 7), D.case(RB, (9, 7))[0])
    assert m.analysis_launch() == dict(DEFAULTS, flow_grid=0, relax_grid=0, strata_grid=0), "a fresh context: the defaults, no launch yet"
    m.set_analysis_launch(3, 5, 7)
    names = list(DEFAULTS)
    for k, name in enumerate(names):
        for bad in (-1, DEFAULTS[name] + 1):
            v = [11, 12, 13]                                               # (the two valid ones are not taken either)
            v[k] = bad
            assert L.smx_set_analysis_launch(m.h, *v) == -2 and f"{name} is {bad}".encode() in L.smx_last_error(m.h)
            assert in_force(m) == (3, 5, 7)
            with pytest.raises(SoilmxError, match=rf"{name} is {bad}.*rc=-2"):
                m.set_analysis_launch(*v)
    m.set_analysis_launch(*DEFAULTS.values())                              # the defaults by their numbers
    assert in_force(m) == tuple(DEFAULTS.values())
    assert L.smx_get_analysis_launch(m.h, None, None) == 0 and L.smx_get_analysis_launch(m.h, b, None) == 0 and list(b) == list(DEFAULTS.values())
    with Ensemble(0) as ens:
        ens.set_analysis_launch(2, 4, 6)
        for k, name in enumerate(names):
            for bad in (-1, DEFAULTS[name] + 1):
                v = [11, 12, 13]
                v[k] = bad
                assert L.smx_ensemble_set_analysis_launch(ens.h, *v) == -2 and f"{name} is {bad}".encode() in L.smx_ensemble_last_error(ens.h)
                assert in_force(ens) == (2, 4, 6)
    DR.assert_same_dispersal(m.dispersal(1, **DISP_ALL), DR.case(RB, (9, 7), 1)[2], "after the refused calls")
    m.close()


def test_a_value_belongs_to_its_owner():
    dims = (33, 47)
    s, drain, want = DR.case(RB, dims, 1)
    cells = dims[0] * dims[1]
    alone = new_map(dims, s)
    with Ensemble(0) as ens:
        ens.set_analysis_launch(1, 1, 1)
        e = ens.add(cfg64(), dims[0], dims[1], seed=1, pool=POOL, initialize=False)
        e.load(s)
        assert in_force(e) == in_force(alone) == tuple(DEFAULTS.values()), "the ensemble's values reach neither a member's own calls nor another context"
        check_dispersal(e, s, want, 1, "a member's own call", 0, blocks(cells))
        check_dispersal(alone, s, want, 1, "a stand-alone context", 0, blocks(cells))
        assert ens.analysis_launch()["flow_grid"] == 0, "no call on the ensemble yet"
        # the other way: a member's and a stand-alone context's values do not reach the ensemble
        ens.set_analysis_launch()
        e.set_analysis_launch(1, 1, 1)
        alone.set_analysis_launch(1, 1, 1)
        DR.assert_same_dispersal((ens.dispersal(1)[0], None), want, "the ensemble at its default beside a capped member")
        ens.soil_totals(4)
        assert in_force(ens) == tuple(DEFAULTS.values())
        assert (ens.analysis_launch()["flow_grid"], ens.analysis_launch()["strata_grid"]) == (blocks(cells), blocks(cells, STRATA_LANES))
        check_dispersal(e, s, want, 1, "the capped member", 1, blocks(cells))
    check_dispersal(alone, s, want, 1, "the capped stand-alone context", 1, blocks(cells))
    alone.close()


def test_the_analyses_without_a_cap_do_not_see_the_values():
    """lakes, drainage, streams, hillslopes, flowpaths, catchments and budget launch a lane per cell or record: the same results,
    each against its restatement, with the three caps at 1 and at the default."""
    dims, t = (33, 47), 4
    s, drain = D.case(RB, dims)
    base, now, _, _ = budget_ref.pair(RB, dims)
    assert base is s
    m, mn = new_map(dims, s), new_map(dims, now)
    _, _, cells, cwant = catchments_ref.case(RB, dims, "every7", 7, 0.25)
    for caps in ((1, 1, 1), (0, 0, 0)):
        m.set_analysis_launch(*caps)
        mn.set_analysis_launch(*caps)
        what = f"{RB} {dims} caps {caps}"
        lakes_ref.assert_same_census(m.lakes(labels=True), lakes_ref.census(s), f"lakes, {what}")
        D.assert_same_drainage(m.drainage(**DRAIN_ALL), drain, f"drainage, {what}")
        streams_ref.assert_same_streams(m.streams(t, order=True, segments=True, reach=True, heads=True), streams_ref.case(RB, dims, t)[2], f"streams, {what}")
        hillslopes_ref.assert_same_hillslopes(m.hillslopes(t, entry=True, hillslope=True, straight=True, diagonal=True, hand=True), hillslopes_ref.case(RB, dims, t)[3],
                                              f"hillslopes, {what}")
        recs, planes = m.flowpaths(profiles=True, terminal=True, straight=True, diagonal=True, drop=True, upstream=True, source=True, stem=True)
        prof = np.concatenate([r["profile"] for r in recs]) if recs else np.zeros(0, np.uint32)
        flowpaths_ref.assert_same_flowpaths((recs, planes, prof), flowpaths_ref.case(RB, dims)[2], f"flowpaths, {what}", nprofile=len(prof))
        crecs, cplanes = m.catchments(cells, bins=7, bin_height=0.25, gauge=True, straight=True, diagonal=True, drop=True)
        catchments_ref.assert_same_catchments((crecs, cplanes, np.array([r["hist"] for r in crecs], np.uint32)), cwant, f"catchments, {what}")
        budget_ref.assert_same_budget(mn.budget(m, 64, dground=True, dheight=True, dsolid=True, dwater=True), budget_ref.want(RB, dims, 64), f"budget, {what}")
        a = m.analysis_launch()
        assert (a["flow_grid"], a["relax_grid"], a["strata_grid"]) == (0, 0, 0), "none of the seven has a capped launch"
    m.close(); mn.close()
