"""Every engine on the MI355X, through the C-ABI, on maps that no tile size divides (tests/oddmaps.py), judged by the oracle: the full state
after each tick and the counters at the end, bit for bit. The launch-level code of soilmx.hip has no twin on the host (tests/hostsim
restates it in another form), so a mistake in its shape-dependent indexing -- the last bitmap word of the classification, grid tiles cut
by both borders, claim tiles of a map of a few tiles, colour lists and flood gates at the border, regions larger than the map -- shows
only here. The oracle itself is held to the compiled reference on these maps in tests/test_oracle_vs_ref.py, the fixture is proven on
host threads in tests/test_oddmaps.py.

Cases run from the friendliest shape (65x63) to the most degenerate (1x70, 70x1, 9x7). Every relaxed case records the launches it took
(PATHS, printed as "[oddmaps]"): none passes through the one-workgroup tail kernel alone without saying so."""
import numpy as np
import pytest

import oddmaps as om
from observe_ref import figures_ref
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilMachine, SoilmxError
from soilmachine_amd.snapshot import compare
from test_gpu_ensemble_observe import assert_figures

pytestmark = pytest.mark.gpu

CASES = [pytest.param(w, s, id=f"{w}-{om.shape_id(s)}") for s in om.DEVICE_ORDER for w in om.WORKLOADS]

# the relaxed engine's variants: launch shape (smx_set_relax_launch), settle mode (smx_set_relax_settle), water generations
RELAXED = {
    "default": ((-1, -1), -1, om.DENSE_GENERATIONS),       # five launches per epoch above 256 running particles, the tail kernel below; settle + floods joined
    "persistent": ((1, 0), -1, om.DENSE_GENERATIONS),      # every epoch through k_relax_epochs (cooperative launch)
    "per-phase": ((0, 0), -1, om.DENSE_GENERATIONS),       # five launches per epoch down to the last particle
    "settle-1": ((-1, -1), 1, om.DENSE_GENERATIONS),       # k_relax_settle, floods in a launch of their own
    "settle-0": ((-1, -1), 0, om.DENSE_GENERATIONS),       # k_relax_filter + k_relax_cascade_flow
    "eight-generations": ((-1, -1), -1, 0),                # the engine's default split: generations of 75 / 38 particles, the tail kernel alone
}
PATHS = {}   # (workload, shape, variant) -> the launches a relaxed case took


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def device(workload, shape, engine):
    cfg = om.cfg_of(workload)
    _, nw, nd, wind = om.WORKLOADS[workload]
    m = Layermap(cfg, shape[0], shape[1], seed=om.SEED, pool=om.POOL, initialize=False, engine=engine)
    m.load(om.start(workload, shape), rand_seed=om.SEED)
    sm = SoilMachine.__new__(SoilMachine)
    sm.cfg, sm.map, sm.nwater, sm.nwind, sm.dowater, sm.dowind = cfg, m, nw, nd, True, wind
    return sm


def run_against_oracle(sm, what, run, keys):
    """tick the device TICKS times against the oracle run `run`; -> the device's counters"""
    snaps, co, st = run
    assert st["guard_violations"] == 0 and co["pool_overflow"] == 0
    for t in range(om.TICKS):
        sm.tick(1, sync=True)
        bad = compare(sm.map.snapshot(), snaps[t])
        assert not bad, f"{what} tick {t}: {bad}"
    cd = sm.map.counters()
    assert {k: cd[k] for k in keys} == {k: co[k] for k in keys}, what
    assert cd["pool_overflow"] == 0
    return cd


@pytest.mark.parametrize("engine", [capi.ENGINE_SERIAL, capi.ENGINE_SPECULATIVE], ids=["serial", "speculative"])
@pytest.mark.parametrize("workload,shape", CASES)
def test_exact_engines_equal_the_oracle(workload, shape, engine):
    run = om.oracle_run(workload, shape, "exact")
    om.must_be_wet(shape, run[1])
    sm = device(workload, shape, engine)
    try:
        run_against_oracle(sm, f"{workload} {om.shape_id(shape)} engine {engine}", run, om.KEYS)
    finally:
        sm.map.close()


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("workload,shape", CASES)
def test_batched_engine_equals_its_restatement(workload, shape, dilate):
    run = om.oracle_run(workload, shape, "batched", dilate)
    om.must_be_wet(shape, run[1])
    sm = device(workload, shape, capi.ENGINE_BATCHED)
    try:
        sm.map.set_batch_dilate(dilate)
        run_against_oracle(sm, f"{workload} {om.shape_id(shape)} batched dilate {dilate}", run, om.KEYS)
        st, bs = run[2], sm.map.batch_stats()
        assert (bs["epochs"], bs["generations"], bs["children_lost"]) == (st["epochs"], st["generations"], 0)
    finally:
        sm.map.close()


def relaxed_case(workload, shape, variant):
    """one relaxed case against the restated schedule -> the launches it took (run once per session, then remembered)"""
    key = (workload, shape, variant)
    if key in PATHS:
        return PATHS[key]
    launch, settle, generations = RELAXED[variant]
    run = om.oracle_run(workload, shape, "relaxed", generations=generations)
    om.must_be_wet(shape, run[1])
    sm = device(workload, shape, capi.ENGINE_RELAXED)
    m = sm.map
    try:
        m.set_relax_wind(0xFFFFFFFF, 4)                      # wind under the exclusive schedule, as the restatement runs it
        m.set_relax_launch(*launch)
        m.set_relax_settle(settle)
        if generations:
            m.set_water_generations(generations)
        run_against_oracle(sm, f"{workload} {om.shape_id(shape)} relaxed {variant}", run, om.RKEYS)
        assert m.batch_stats()["children_lost"] == 0
        t = m.timing()
        path = dict(m.relax_settle_stats(), **m.relax_flood_flow_stats(), epochs=m.batch_stats()["epochs"],
                    persistent_launches=t["launches_kernel_epochs"], tail_launches=t["launches_kernel_tail"], step_launches=t["launches_step_water"])
    finally:
        m.close()
    path["dense_epochs"] = path["epochs_fused"] + path["epochs_split"]
    print("[oddmaps]", workload, om.shape_id(shape), variant, path)
    PATHS[key] = path
    return path


@pytest.mark.parametrize("variant", list(RELAXED))
@pytest.mark.parametrize("workload,shape", CASES)
def test_relaxed_engine_equals_its_restatement(workload, shape, variant):
    p = relaxed_case(workload, shape, variant)
    # Which launches a case takes follows from the particle counts, not from the map: one generation of 600 / 300 particles is above the
    # 256 of the tail kernel on every shape, eight generations of 75 / 38 are below it and so is every nested generation of these maps.
    if variant == "eight-generations":
        assert p["tail_launches"] > 0 and p["dense_epochs"] == 0 and p["persistent_launches"] == 0, p
        return
    if variant == "persistent":
        assert p["persistent_launches"] > 0 or p["dense_epochs"] > 0, p      # (per-phase launches where the cooperative launch is refused)
        return
    assert p["dense_epochs"] > 0 and p["step_launches"] > 0, p               # (on every shape, the sub-tile ones included)
    if variant == "per-phase":
        assert p["tail_launches"] == 0, p
    if variant == "settle-1":
        assert p["epochs_fused"] > 0 and p["epochs_joined"] == 0 and p["epochs_split"] == 0, p
    if variant == "settle-0":
        assert p["epochs_split"] > 0 and p["epochs_fused"] == 0 and p["epochs_joined"] == 0 and p["crowded_cells"] == 0, p


# the settle paths by name: which odd-shape case covers which launch
SETTLE_PATHS = {
    "joined (k_relax_settle_floods)": [("default", (33, 47), "default"), ("default", (9, 7), "per-phase")],
    "one launch (k_relax_settle)": [("default", (33, 47), "settle-1"), ("rgps", (17, 19), "settle-1")],
    "two launches (k_relax_filter + k_relax_cascade_flow)": [("default", (33, 47), "settle-0"), ("rgps", (1, 70), "settle-0")],
}


@pytest.mark.parametrize("path", list(SETTLE_PATHS))
def test_each_settle_path_is_taken_on_an_odd_shape(path):
    for workload, shape, variant in SETTLE_PATHS[path]:
        p = relaxed_case(workload, shape, variant)
        if path.startswith("joined"):
            assert p["epochs_joined"] > 0 and p["epochs_split"] == 0, (workload, shape, variant, p)
            if min(shape) >= 7 and variant == "per-phase":          # (every epoch is a joined one: the oracle's floods all act there)
                assert p["floods_acted"] > 0, (workload, shape, variant, p)
        elif path.startswith("one launch"):
            assert p["epochs_fused"] > 0 and p["epochs_joined"] == 0 and p["epochs_split"] == 0, (workload, shape, variant, p)
        else:
            assert p["epochs_split"] > 0 and p["epochs_fused"] == 0, (workload, shape, variant, p)


def test_ensemble_members_of_every_shape_equal_the_oracle():
    """one ensemble, a member of every shape and both soils, ticked together: each member against the ORACLE (k_ens_classify and the
    other k_ens_* kernels with per-member bounds before an independent judge), then figures() against the snapshot's own figures"""
    cases = [(w, s) for s in om.DEVICE_ORDER for w in om.WORKLOADS]
    want = []
    for w, s in cases:                                        # (every member runs its wind phase: the default workload with no particles)
        _, nw, nd, _ = om.WORKLOADS[w]
        o = om.fresh_oracle(w, s)
        snaps = []
        for _ in range(om.TICKS):
            o.tick(nw, nd, True, True)
            snaps.append(o.snapshot())
        want.append((snaps, o.counters()))
        o.close()
    with Ensemble(0) as ens:
        mem = []
        for w, s in cases:
            m = ens.add(om.cfg_of(w), s[0], s[1], seed=om.SEED, pool=om.POOL, initialize=False)
            m.load(om.start(w, s), rand_seed=om.SEED)
            mem.append(m)
        nwater = [om.WORKLOADS[w][1] for w, _ in cases]
        nwind = [om.WORKLOADS[w][2] for w, _ in cases]
        for t in range(om.TICKS):
            ens.tick(nwater, nwind, True, True)
            ens.sync()
            for (w, s), m, (snaps, _) in zip(cases, mem, want):
                bad = compare(m.snapshot(), snaps[t])
                assert not bad, f"member {w} {om.shape_id(s)} tick {t}: {bad}"
        figs = ens.figures()
        for (w, s), m, (snaps, co), f in zip(cases, mem, want, figs):
            cd = m.counters()
            assert {k: cd[k] for k in om.KEYS} == {k: co[k] for k in om.KEYS}, (w, s)
            ref = figures_ref(snaps[-1])
            ref["rand_calls"], ref["live_sections"] = co["rand_calls"], snaps[-1].nsec
            assert_figures(f, ref, f"member {w} {om.shape_id(s)}")


@pytest.mark.parametrize("shape", [(33, 47), (9, 7), (1, 70), (70, 1)], ids=om.shape_id)
def test_readers_equal_the_oracle(shape):
    """heights, surface types and normals of the wet start state (on 1x70 and 70x1 no cell has a neighbour on both axes, on 9x7 most
    cells take the k = 1, 2 border rule), and Layermap::height(vec2). The reference reads the cells (px + 1, py + 1) without a check, so
    a position is defined only in [0, dimx - 1) x [0, dimy - 1): there the reader equals the oracle, anywhere else -- every position of a
    map one cell wide -- the call is refused, reads nothing and leaves the context usable."""
    dx, dy = shape
    m = device("rgps", shape, capi.ENGINE_SERIAL).map
    o = om.fresh_oracle("rgps", shape)
    try:
        assert np.array_equal(bits(m.heights()), bits(o.heights()))
        surf = np.array([o.L.so_surface(o.h, x, y) for x in range(dx) for y in range(dy)], np.uint32)
        assert np.array_equal(m.surface(), surf)
        ref = np.zeros((dx * dy, 3), np.float32)
        tmp = np.zeros(3, np.float32)
        for x in range(dx):
            for y in range(dy):
                o.L.so_normal(o.h, x, y, tmp.ctypes.data)
                ref[x * dy + y] = tmp
        assert np.array_equal(bits(m.normals()), bits(ref))
        outside = [(dx - 1.0, 0.0), (0.0, dy - 1.0), (dx - 0.5, dy - 0.5), (-0.25, 0.0), (0.0, -1.0), (float(dx), 0.0), (float("nan"), 0.0)]
        if min(shape) >= 2:
            rng = np.random.default_rng(0)
            pos = (rng.random((2000, 2)) * (np.array([dx, dy]) - 1.001)).astype(np.float32)
            pos[:50] = np.floor(pos[:50])                      # exact integer positions too
            pos[50] = (dx - 2, dy - 2)                         # the last cell a position may start from
            pos[51] = np.nextafter(np.float32(dx - 1), np.float32(0)), np.nextafter(np.float32(dy - 1), np.float32(0))
            want = np.array([o.L.so_height_bilinear(o.h, float(p[0]), float(p[1])) for p in pos])
            assert np.array_equal(bits(m.heights_bilinear(pos)), bits(want))
        else:
            outside += [(0.0, 0.0), (0.0, 3.5), (3.5, 0.0), (0.5, 0.5)]     # one cell wide: no position has its four cells
        for p in outside:
            with pytest.raises(SoilmxError, match="outside"):
                m.heights_bilinear(np.array([[0.0, 0.0], p] if min(shape) >= 2 else [p], np.float32))
        assert np.array_equal(bits(m.heights()), bits(o.heights()))          # the refused calls left the context as it was
    finally:
        m.close()
        o.close()
