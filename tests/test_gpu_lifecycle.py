"""Who owns a context's memory (soilmachine_amd/csrc/soil_devmem.h), seen from outside on a real MI355X: buffers that grew between
two ticks leave the results as a fresh context computes them, and every kind of object can be created, used and destroyed in every
order that has a free path of its own, after which the device still computes the committed golden state. Nothing here provokes a
failure: the out-of-memory paths are exercised on the CPU (tests/test_devmem_host.py)."""
import numpy as np
import pytest

from common import SNAP_CASES, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.lbm import LbmWind
from soilmachine_amd.machine import Layermap, SoilMachine
from soilmachine_amd.snapshot import compare
from strips_ref import LibStripRank, StripGeometry, ThreadComm, run_threads

pytestmark = pytest.mark.gpu
DIG = digests()
N = 64
POOL = 1 << 20            # sections per context: 250 times what the 64^2 goldens hold, a tenth of the default's allocation and upload
ALL_ENGINES = [capi.ENGINE_SERIAL, capi.ENGINE_SPECULATIVE, capi.ENGINE_BATCHED, capi.ENGINE_RELAXED]
# work a tick has done, whichever way it was scheduled
WORK = ("steps_water_top", "steps_water_all", "steps_wind", "nested_particles", "floods", "cascade_calls", "cascade_transfers", "wcascade_calls", "pool_overflow")


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def assert_device_still_computes_the_golden():
    """A fresh context reproduces the 64^2 golden after five ticks: snapshot bit for bit, and the device's own digest."""
    soil, seed, dowind, _ = SNAP_CASES["default64"]
    d = DIG["default64"]
    sm = SoilMachine(load_cfg(soil), N, seed=seed, nwater=d["nwater"], nwind=d["nwind"], dowind=dowind, pool=POOL)
    sm.tick(5, sync=True)
    want = golden_snapshot("default64", 5)
    bad = compare(sm.map.snapshot(), want)
    assert not bad, bad
    g, w = sm.map.digest(), want.digest()
    assert (g["sumh"], g["nsec"], g["typehash"], g["rand_calls"]) == (w["sumh"], w["nsec"], w["typehash"], want.rand_calls)
    sm.map.close()


def tick(m, nwater, nwind):
    m._chk(m.L.smx_tick(m.h, nwater, nwind, 1, 1))
    m.sync()


def state(m):
    c = m.counters()
    return m.digest(), c["rand_calls"], c["pool_free"], {k: c[k] for k in WORK}


# ---------------------------------------------------------------- regrown buffers do not change results
@pytest.mark.parametrize("engine", ALL_ENGINES)
def test_regrown_buffers_do_not_change_results(engine):
    """A ticks once with few particles (every engine buffer at its floor size), loads S and ticks with enough particles to regrow
    them; B is fresh, loads S and runs the large tick only. Device digest, rand() draws, free pool and the work done are equal,
    and so are the full states."""
    cfg = cfg64()
    S = golden_snapshot("default64", 5)
    # batched / relaxed: above the 4096-slot floor and the 2 x 4096 draws floor; speculative (and serial): above the 1024-particle floor
    big = 5000 if engine in (capi.ENGINE_BATCHED, capi.ENGINE_RELAXED) else 1500
    a = Layermap(cfg, N, N, seed=0, pool=POOL, engine=engine)
    tick(a, 40, 40)
    b = Layermap(cfg, N, N, seed=0, pool=POOL, engine=engine, initialize=False)
    steps = [None, 1024] if engine == capi.ENGINE_SPECULATIVE else [None]    # then smx_set_spec_limits: the buffers are reallocated at the same particle count
    for m in (a, b):
        m.load(S, rand_seed=0)
    for maxnest in steps:
        got = []
        for m in (a, b):
            if maxnest is not None:
                m._chk(m.L.smx_set_spec_limits(m.h, 0, maxnest))
            before = m.counters()
            tick(m, big, big)
            dg, rc, pf, work = state(m)
            got.append((dg, rc, pf, {k: work[k] - before[k] for k in WORK}))
            drawn = rc - before["rand_calls"]
        assert got[0] == got[1], f"maxnest {maxnest}"
        # both phases ran at the large count: every particle is born from two draws. (No soil of default.soil can be suspended, so a
        # wind particle ends at birth, wind.h:56-57, and steps_wind stays 0; its slot and its draws are what the buffers grow for.)
        assert got[0][3]["pool_overflow"] == 0 and got[0][3]["steps_water_top"] > 0 and drawn >= 2 * big + 2 * big
        bad = compare(a.snapshot(), b.snapshot())
        assert not bad, bad
    a.close(); b.close()


# ---------------------------------------------------------------- create, use, destroy
def test_destroy_a_context_that_never_ticked():
    cfg = cfg64()
    Layermap(cfg, N, N, seed=0, pool=POOL).close()
    Layermap(cfg, N, N, seed=0, pool=POOL, initialize=False).close()
    assert_device_still_computes_the_golden()


@pytest.mark.parametrize("engine", ALL_ENGINES)
def test_destroy_a_context_after_one_tick(engine):
    m = Layermap(cfg64(), N, N, seed=0, pool=POOL, engine=engine)
    tick(m, 100, 100)
    m.close()
    assert_device_still_computes_the_golden()


def test_destroy_a_context_after_the_read_side_scratch_was_made():
    cfg = cfg64()
    m = Layermap(cfg, N, N, seed=0, pool=POOL)
    colors = np.linspace(0.05, 0.95, 4 * len(cfg.soils), dtype=np.float32).reshape(-1, 4)
    h = m.heights()                                                  # smx_read_heights: the plane scratch
    v = m.vertices(colors)                                           # smx_fill_vertices: colour table and whole-map scratch
    one = m.vertex(3, 5, colors, cut=40.0)                           # smx_fill_vertex_cut: the one-block scratch
    assert np.isfinite(h).all() and np.isfinite(v).all() and np.isfinite(one).all()
    assert np.array_equal(m.vertex(3, 5, colors), v[3 * N + 5]), "one column's vertex = its record in the whole-map stream"
    m.close()
    assert_device_still_computes_the_golden()


def test_destroy_a_strip_pair_on_the_loopback_transport():
    """Two strip contexts, host transports attached, one small tick (exchange buffers, pinned staging), destroyed with the
    transports still attached. 224 x 64: the library refuses strips narrower than two seam zones of 48 columns plus 16."""
    cfg = cfg64()
    dimx, G = 224, 2
    geom = StripGeometry(dimx, G)
    s0 = Layermap(cfg, dimx, N, seed=0, pool=POOL).snapshot()
    ms = []
    for r in range(G):
        m = Layermap(cfg, dimx, N, seed=0, pool=POOL, initialize=False, engine=capi.ENGINE_BATCHED, x_range=geom.held(r, N))
        m.load(s0, rand_seed=0)
        ms.append(m)
    comms = ThreadComm.world(G)
    ranks = [None] * G

    class R:
        def __init__(self, r): self.r, self.comm = r, comms[r]

    def attach_and_tick(o):
        ranks[o.r] = LibStripRank(ms[o.r], comms[o.r], geom)
        ranks[o.r].tick(60, 30, True, True)
    run_threads([R(r) for r in range(G)], attach_and_tick)
    assert ranks[0].stats["messages"] > 0
    for m in ms:
        m.close()
    assert_device_still_computes_the_golden()


def test_destroy_an_ensemble_grown_past_its_first_table_observed_and_forked():
    cfg = cfg64()
    pool = 1 << 16
    ens = Ensemble()
    for s in range(3):
        ens.add(cfg, N, N, seed=s, pool=pool)
    ens.tick(20, 20)                                                 # the 64-entry table in use
    first = ens.figures()
    for s in range(3, 70):                                           # crosses it: both tables are replaced
        ens.add(cfg, N, N, seed=s, pool=pool)
    assert ens.size() == 70
    f = ens.figures()
    assert len(f) == 70 and f[:3] == first, "the first members' states came through the table swap"
    ens.tick(20, 20)
    st = ens.plane_stats("height")
    assert st["mean"].shape == (N * N,) and np.isfinite(st["mean"]).all() and (st["vmin"] <= st["vmax"]).all() and (st["nonzero"] <= 70).all()
    made = ens.fork(ens.members[0], 2, seeds=[11, 12])
    assert ens.size() == 72
    f = ens.figures()
    assert (f[70]["sumh"], f[70]["nsec"], f[70]["typehash"]) == (f[0]["sumh"], f[0]["nsec"], f[0]["typehash"]) and len(made) == 2
    ens.tick(20, 20)
    ens.sync()
    ens.close()
    assert_device_still_computes_the_golden()


def test_destroy_an_lbm_lattice():
    m = Layermap(cfg64(), N, N, seed=0, pool=POOL)
    g = LbmWind(8, 8, 8)
    g.boundary_from_map(m, 1.0, 1.0, 1.0)                            # (grows the map context's plane scratch from the lattice's call)
    g.initialize()
    g.step(1)
    rho, v, _ = g.read()
    assert rho.shape == (512,) and v.shape == (512, 4)
    g.close()
    m.close()
    assert_device_still_computes_the_golden()


# ---------------------------------------------------------------- a member is the ensemble's to free
def test_smx_destroy_still_refuses_an_ensemble_member():
    cfg = cfg64()
    ens = Ensemble()
    ms = [ens.add(cfg, N, N, seed=s, pool=1 << 16) for s in range(2)]
    ens.tick(30, 30)
    before = ens.figures()
    L = ens.L
    L.smx_destroy(ms[0].h)                                           # returns without freeing anything
    assert b"member of an ensemble" in L.smx_last_error(ms[0].h)
    assert ens.size() == 2 and ens.figures() == before, "digests unchanged"
    ens.tick(30, 30)                                                 # ... and it still ticks, to the state a context of its own reaches
    ens.sync()
    for s in range(2):
        ref = Layermap(cfg, N, N, seed=s, pool=1 << 16)
        for _ in range(2):
            tick(ref, 30, 30)
        bad = compare(ms[s].snapshot(), ref.snapshot())
        assert not bad, (s, bad)
        ref.close()
    ens.close()
    assert_device_still_computes_the_golden()
