"""The sediment budget on a real MI355X (smx_budget / smx_ensemble_budget; k_budget_fold, k_budget_where): the base in one map, now in
another, and every record field and every plane equals the plain-loop restatement tests/budget_ref.py bit for bit. No test here feeds
the device a corrupt chain: that is the host bodies' business (tests/test_budget_host.py)."""
import ctypes as C

import numpy as np
import pytest

import budget_ref as R
import strata_ref as S
from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from test_budget_host import GOLDEN_PAIRS, hand_pair

pytestmark = pytest.mark.gpu
DIG = digests()
POOL = 1 << 18
ALL = dict(dground=True, dheight=True, dsolid=True, dwater=True)
BSZ, SSZ = C.sizeof(capi.BudgetBasin), C.sizeof(capi.BudgetSoil)
NOPLANES = (None, None, None, None)


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def maps_of(cfg, base, now):
    a = Layermap(cfg, base.dimx, base.dimy, seed=0, pool=POOL, initialize=False)
    b = Layermap(cfg, base.dimx, base.dimy, seed=0, pool=POOL, initialize=False)
    a.load(base); b.load(now)
    return a, b


def state(m):
    return m.digest(), m.counters()


# ---------------------------------------------------------------- 1. the golden pairs
@pytest.mark.parametrize("case,t0,t1", GOLDEN_PAIRS, ids=lambda v: str(v))
def test_golden_pair(case, t0, t1):
    base, now = golden_snapshot(case, t0), golden_snapshot(case, t1)
    cfg = load_cfg(SNAP_CASES[case][0])
    mb, mn = maps_of(cfg, base, now)
    before = state(mb), state(mn)
    got = mn.budget(mb, **ALL)
    nt = len(got[1])
    assert nt == len(cfg.soils) > int(max(base.type.max(), now.type.max())), "ntypes None: the soil table's length"
    want = R.budget(base, now, nt)
    R.assert_same_budget(got, want, f"{case} t{t0} -> t{t1}")
    R.assert_invariants(base, now, *got, what=f"{case} t{t0} -> t{t1}")
    assert all(r[f] == r[f + "_q40"] / 2 ** 40 for r in got[0] for f in ("eroded", "deposited")) and all(r["net"] == (r["deposited_q40"] - r["eroded_q40"]) / 2 ** 40 for r in got[0])
    # the basins are the base's, and the soil table is the change of what soil_totals() says of the two maps
    assert [(r["first_cell"], r["cells"]) for r in got[0]] == [(b["first_cell"], b["cells"]) for b in mb.drainage()]
    tb, tn = mb.soil_totals(nt), mn.soil_totals(nt)
    for t, q in enumerate(got[1]):
        assert q["gained_q40"] - q["lost_q40"] == tn[t]["volume_q40"] - tb[t]["volume_q40"] and q["held_gained_q40"] - q["held_lost_q40"] == tn[t]["held_q40"] - tb[t]["held_q40"], t
        assert q["surfaced"] - q["covered"] == tn[t]["top_cells"] - tb[t]["top_cells"], t
    # the other way round: what was eroded is deposited
    back = mb.budget(mn, nt)
    assert sum(r["eroded_q40"] for r in back[0]) == sum(r["deposited_q40"] for r in got[0]) and [q["lost_q40"] for q in back[1]] == [q["gained_q40"] for q in got[1]]
    assert (state(mb), state(mn)) == before, "a call changed a map, a counter or a generator"
    mb.close(); mn.close()


# ---------------------------------------------------------------- 2. the synthetic pairs and the hand-built one
@pytest.mark.parametrize("dims", R.PAIR_DIMS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_synthetic_pairs(dims):
    cfg = cfg64()
    mb = Layermap(cfg, dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    mn = Layermap(cfg, dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    for name in R.PAIR_INPUTS:
        base, now, notes, _ = R.pair(name, dims)
        mb.load(base); mn.load(now)
        got = mn.budget(mb, 64, **ALL)
        R.assert_same_budget(got, R.want(name, dims, 64), f"{name} {dims}")
        R.assert_invariants(base, now, *got, what=f"{name} {dims}")
        R.assert_same_budget(mn.budget(mb, 5), R.want(name, dims, 5), f"{name} {dims}, 5 types: the others count in S and are absent from the table")
        if "tie" in notes and name == "cone":
            assert got[0][0]["cut_cell"] == notes["tie"][0] and got[0][0]["cut_max"] == R.TIE, "of two cells that tie the smaller index wins"
    mb.close(); mn.close()


def test_hand_built_pair():
    base, now = hand_pair()
    mb, mn = maps_of(cfg64(), base, now)
    basins, soils, planes = mn.budget(mb, 64, **ALL)
    Q = 1 << 40
    assert [(r["first_cell"], r["cells"], r["lowered_cells"], r["raised_cells"], r["resurfaced_cells"], r["eroded_q40"], r["deposited_q40"], r["water_gained_q40"],
             r["water_lost_q40"], r["cut_max"], r["cut_cell"], r["fill_max"], r["fill_cell"], r["flags"], r["net"]) for r in basins] == \
        [(0, 252, 2, 1, 2, Q // 2, Q // 2, Q // 8, 0, 0.25, 17, 0.5, 40, 0, 0.0), (255, 4, 1, 1, 2, Q // 2, Q, 0, 0, 0.5, 255, 1.0, 238, 0, 0.5)]
    assert (soils[1]["lost_q40"], soils[1]["cells_lost"], soils[1]["covered"], soils[1]["net"]) == (Q, 3, 4, -1.0)
    assert (soils[2]["gained_q40"], soils[2]["held_gained_q40"], soils[2]["surfaced"]) == (Q // 2, Q // 4, 1) and soils[63]["gained_q40"] == Q and soils[0]["gained_q40"] == Q // 8
    R.assert_same_budget((basins, soils, planes), R.budget(base, now, 64), "hand-built")
    mb.close(); mn.close()


# ---------------------------------------------------------------- 3. a live run; a copy; the planes one by one, records only, caps
def test_live_run_against_the_state_kept_before_it():
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), 64, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=1 << 20)
    m = sm.map
    base = Layermap(m.cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    base.copy_from(m)
    R.assert_all_zero(*m.budget(base, **ALL), what="against the copy just taken")
    sm.tick(3)
    got = m.budget(base, **ALL)                                # right behind the ticks, no sync between
    m.sync()
    sb, sn = base.snapshot(), m.snapshot()
    want = R.budget(sb, sn, len(got[1]))
    R.assert_same_budget(got, want, "default64, three ticks from the copy")
    R.assert_invariants(sb, sn, *got, what="default64, three ticks")
    assert sum(r["lowered_cells"] for r in got[0]) > 500 and sum(r["raised_cells"] for r in got[0]) > 500, "the ticks moved the land"
    # each plane alone, records only, caps below and above the count -- the soil table covers the whole map whatever cap is
    nb = len(want[0])
    for p in ALL:
        R.assert_same_budget(m.budget(base, **{p: True}), want, f"the {p} plane alone")
    R.assert_same_budget(m.budget(base), want, "records only")
    for cap in (0, 1, nb - 1, nb + 5):
        R.assert_same_budget(m.budget(base, cap=cap, dsolid=True), want, f"cap {cap}", cap=cap)
    n = C.c_uint32()
    assert m.L.smx_budget(m.h, base.h, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES) == 0 and n.value == nb, "counting"
    short = np.full(3 * nb + 1, 0xABABABAB, np.uint32)         # a caller compiled against a 12-byte struct
    assert m.L.smx_budget(m.h, base.h, capi.ptr(short), 12, nb, C.byref(n), None, 0, 0, *NOPLANES) == 0
    assert [tuple(int(x) for x in short[3 * k:3 * k + 3]) for k in range(nb)] == [(r["first_cell"], r["cells"], r["lowered_cells"]) for r in want[0]] and short[-1] == 0xABABABAB
    m.close(); base.close()


# ---------------------------------------------------------------- 4. an ensemble against the source of its fork
def test_ensemble_members_against_the_source_of_the_fork():
    soil, seed, dowind, _ = SNAP_CASES["rgps64"]
    cfg, d = load_cfg(soil), DIG["rgps64"]
    nt = len(cfg.soils)
    base = Layermap(cfg, 64, 64, seed=0, pool=POOL, initialize=False)
    base.load(golden_snapshot("rgps64", 3))
    with Ensemble(0) as ens:
        assert ens.budget(base, nt) == []
        assert ens.L.smx_ensemble_budget(ens.h, base.h, None, BSZ, 0, None, None, 0, 0) == 0, "an empty ensemble: 0, nothing written"
        mem = ens.fork(base, 3, seeds=[21, 22, 23], pool=POOL)
        ens.tick(d["nwater"], d["nwind"], n=2)
        got = ens.budget(base, nt)                             # right behind the ticks
        own = [m.budget(base, nt) for m in mem]
        assert len(got) == 3
        for i in range(3):
            R.assert_same_budget(got[i], own[i], f"member {i}: the ensemble call against its own call")
        assert len({str(g[0]) for g in got}) == 3, "three seeds, three budgets"
        sb = base.snapshot()
        R.assert_same_budget(got[1], R.budget(sb, mem[1].snapshot(), nt), "member 1 against the restatement")
        # a fourth member after the first call: the scratch regrows; cap below the count
        mem += ens.fork(mem[0], 1, seeds=[24], pool=POOL)
        again = ens.budget(base, nt)
        for i in range(3):
            R.assert_same_budget(again[i], got[i], f"member {i} after the ensemble grew")
        R.assert_same_budget(again[3], got[0], "the fork of member 0 before it is ticked")
        cut = ens.budget(base, nt, cap=2)
        assert [len(c[0]) for c in cut] == [2] * 4 and all(c[1] == a[1] for c, a in zip(cut, again))
        R.assert_same_budget(cut[2], again[2], "cap 2", cap=2)
        # refused: the base among the members, a member of other dimensions
        with pytest.raises(SoilmxError, match="member 1 itself"):
            ens.budget(mem[1], nt)
        odd = ens.add(cfg64(), 33, 47, seed=1, pool=1 << 16)
        with pytest.raises(SoilmxError, match="member 4 is 33x47"):
            ens.budget(base, nt)
        n = C.c_uint32(7)
        assert ens.L.smx_ensemble_budget(ens.h, base.h, None, BSZ, 0, C.byref(n), None, 0, 0) == -2 and n.value == 7
        ens.remove(odd)
        R.assert_same_budget(ens.budget(base, nt)[3], again[3], "after the refused calls")
    base.close()


# ---------------------------------------------------------------- 5. errors
def test_refused_arguments():
    L = capi.load()
    n = C.c_uint32(7)
    cfg = cfg64()
    base, now, _, _ = R.pair("random_bernoulli20", (33, 47))
    want = R.want("random_bernoulli20", (33, 47), 64)
    mb, mn = maps_of(cfg, base, now)
    soils = (capi.BudgetSoil * 64)()

    def refused(text, *args):
        assert L.smx_budget(*args) == -2 and n.value == 7, text
        assert text.encode() in L.smx_last_error(args[0]), (text, L.smx_last_error(args[0]))

    assert L.smx_budget(None, mb.h, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES) == -2 and L.smx_ensemble_budget(None, mb.h, None, BSZ, 0, C.byref(n), None, 0, 0) == -2
    refused("base is null", mn.h, None, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES)
    refused("the context itself", mn.h, mn.h, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES)
    refused("struct_size is 0", mn.h, mb.h, None, 0, 0, C.byref(n), None, 0, 0, *NOPLANES)
    refused("nbasins is null", mn.h, mb.h, None, BSZ, 0, None, None, 0, 0, *NOPLANES)
    refused("out is null", mn.h, mb.h, None, BSZ, 3, C.byref(n), None, 0, 0, *NOPLANES)
    refused("ntypes is 0", mn.h, mb.h, None, BSZ, 0, C.byref(n), soils, SSZ, 0, *NOPLANES)
    refused("ntypes is 65", mn.h, mb.h, None, BSZ, 0, C.byref(n), soils, SSZ, 65, *NOPLANES)
    refused("soil_struct_size is 0", mn.h, mb.h, None, BSZ, 0, C.byref(n), soils, 0, 5, *NOPLANES)
    other = Layermap(cfg, 47, 33, seed=0, pool=POOL, initialize=False)
    refused("the context is 33x47, the base is 47x33", mn.h, other.h, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES)
    with pytest.raises(SoilmxError, match="47x33"):
        mn.budget(other)
    other.close()
    strip = Layermap(cfg, 128, 64, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=(0, 64))
    refused("strip context", strip.h, mb.h, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES)
    refused("the base is a strip context", mn.h, strip.h, None, BSZ, 0, C.byref(n), None, 0, 0, *NOPLANES)
    strip.close()
    R.assert_same_budget(mn.budget(mb, 64, **ALL), want, "after the refused calls")
    mb.close(); mn.close()
