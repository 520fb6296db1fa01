"""Ensembles (smx_ensemble_*, soilmachine_amd/ensemble.py) on a real MI355X: many exact maps ticked together, each member
bit-identical to a standalone SERIAL context driven with the same inputs, hence to the reference's golden states."""
import ctypes as C

import pytest

from common import SNAP_CASES, case_dims, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilmxError
from soilmachine_amd.snapshot import compare
from soilmachine_amd.soilfile import layers_array

pytestmark = pytest.mark.gpu
DIG = digests()


def rand_state(m) -> tuple:
    ring, idx, calls = (C.c_uint32 * 31)(), C.c_uint32(), C.c_uint64()
    m._chk(m.L.smx_get_rand_state(m.h, ring, C.byref(idx), C.byref(calls)))
    return tuple(ring), int(idx.value), int(calls.value)


def standalone_tick(m, nwater, nwind, dowater, dowind):
    m._chk(m.L.smx_tick(m.h, int(nwater), int(nwind), int(dowater), int(dowind)))


def assert_same(a, b, what, counters=True):
    bad = compare(a.snapshot(), b.snapshot())
    assert not bad, f"{what}: {bad}"
    assert rand_state(a) == rand_state(b), f"{what}: rand() generator"
    if counters:
        assert a.counters() == b.counters(), f"{what}: counters"


def digest_case(case):
    d = DIG[case]
    cfg = load_cfg(d["soil"])
    dimx, dimy = case_dims(d, cfg)
    kw = d["kw"]
    nwind = d["nwind"] if kw.get("wind", True) else 0
    return cfg, dimx, dimy, kw.get("seed", 0), d["nwater"], nwind, d["ticks"]


# ---------------------------------------------------------------- 1. reference digests, mixed members in one ensemble
DIGEST_MEMBERS = ["default64", "default64s7", "rgps64", "rocksand48x80", "painted64", "default256_t20", "default256_t20_wind",
                  "sand256_t10", "bigbutte2_128_t10"]


def test_mixed_members_reproduce_reference_digests():
    with Ensemble(0) as ens:
        runs = []
        for case in DIGEST_MEMBERS:
            cfg, dimx, dimy, seed, nwater, nwind, ticks = digest_case(case)
            runs.append((case, ens.add(cfg, dimx, dimy, seed=seed), nwater, nwind, ticks))
        for t in range(max(r[4] for r in runs)):
            ens.tick([nw if t < tk else None for _, _, nw, _, tk in runs], [nd for _, _, _, nd, _ in runs])
        ens.sync()
        for case, m, _, _, _ in runs:
            d = DIG[case]
            s = m.snapshot()
            g = s.digest()
            assert (g["nsec"], g["typehash"], g["sumh"], s.rand_calls) == (d["nsec"], d["typehash"], d["sumh"], d["rand_calls"]), case
            c = m.counters()
            assert (c["steps_water_top"], c["steps_wind"]) == (d["steps_water_top"], d["steps_wind"]), case
            assert c["pool_overflow"] == 0, case


# ---------------------------------------------------------------- 2. golden snapshots at intermediate ticks
def test_members_reproduce_golden_snapshots():
    with Ensemble(0) as ens:
        runs = []
        for case in sorted(SNAP_CASES):
            soil, seed, dowind, ticks = SNAP_CASES[case]
            cfg = load_cfg(soil)
            d = DIG[case]
            dimx, dimy = case_dims(d, cfg)
            runs.append((case, ens.add(cfg, dimx, dimy, seed=seed), d["nwater"], d["nwind"] if dowind else 0, ticks))
        checked = 0
        for t in range(max(r[4][-1] for r in runs) + 1):
            ens.sync()
            for case, m, _, _, ticks in runs:
                if t in ticks:
                    bad = compare(m.snapshot(), golden_snapshot(case, t))
                    assert not bad, f"{case} tick {t}: {bad}"
                    checked += 1
            ens.tick([nw if t < ticks[-1] else None for _, _, nw, _, ticks in runs], [nd for _, _, _, nd, _ in runs])
        assert checked == sum(len(r[4]) for r in runs)


# ---------------------------------------------------------------- 3. ensemble == standalone contexts, bit for bit
@pytest.mark.parametrize("dowater,dowind", [(1, 1), (1, 0), (0, 1)])
def test_ensemble_equals_standalone_contexts(dowater, dowind):
    rgps, rocksand = load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")
    specs = [(rgps, 64, 64, s) for s in range(32)] + [(rocksand, 33, 47, 7)]   # 47 % 8 != 0: the scalar classification
    nwater = [60 + 5 * (i % 7) for i in range(len(specs))]
    nwind = [20 + 3 * (i % 5) for i in range(len(specs))]
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, dx, dy, seed=s, pool=64 * dx * dy) for cfg, dx, dy, s in specs]
        ref = [Layermap(cfg, dx, dy, seed=s, pool=64 * dx * dy) for cfg, dx, dy, s in specs]
        try:
            for i in range(len(specs)):
                assert_same(mem[i], ref[i], f"member {i} before the first tick")
            for t in range(6):
                out = {3, 17} if t in (2, 4) else set()
                ens.tick([None if i in out else nwater[i] for i in range(len(specs))], nwind, dowater, dowind)
                for i, r in enumerate(ref):
                    if i not in out:
                        standalone_tick(r, nwater[i], nwind[i], dowater, dowind)
                ens.sync()
                for i in range(len(specs)):
                    assert_same(mem[i], ref[i], f"member {i} after tick {t}")
        finally:
            for r in ref:
                r.close()


# ---------------------------------------------------------------- 4. members stay ordinary contexts
def test_members_save_restore_and_tick_alone(tmp_path):
    cfg = load_cfg("rockgravelpebblessand.soil")
    nw, nd = 80, 40
    with Ensemble(0) as ens:
        a = ens.add(load_cfg("default.soil"), 64, 64, seed=0, pool=1 << 18)
        m = ens.add(cfg, 64, 64, seed=3, pool=1 << 18)
        whole = Layermap(cfg, 64, 64, seed=3, pool=1 << 18)
        for _ in range(3):
            ens.tick(nw, nd)
            standalone_tick(whole, nw, nd, 1, 1)
        path = str(tmp_path / "member.smx")
        m.save(path)                                          # (queued behind the ensemble's ticks on the shared stream)
        resumed = Layermap(cfg, 64, 64, seed=99, pool=1 << 18, initialize=False)
        assert resumed.restore(path)                          # the rand() generator comes with the file
        standalone_tick(m, nw, nd, 1, 1)                      # smx_tick on the member itself, between two ensemble ticks
        standalone_tick(resumed, nw, nd, 1, 1)
        standalone_tick(whole, nw, nd, 1, 1)
        for _ in range(2):
            ens.tick(nw, nd)
            standalone_tick(resumed, nw, nd, 1, 1)
            standalone_tick(whole, nw, nd, 1, 1)
        ens.sync()
        assert_same(m, whole, "member after save, smx_tick and two more ensemble ticks")
        # (a checkpoint carries the map and the generator, not the step counters: those start again at the restore)
        assert_same(resumed, whole, "context restored from the member's checkpoint", counters=False)
        m.close()                                             # frees nothing: the ensemble owns the member
        assert ens.size() == 2 and a.counters()["steps_water_top"] > 0
        whole.close()
        resumed.close()


def test_smx_destroy_on_a_member_is_a_refused_no_op():
    L = capi.load()
    with Ensemble(0) as ens:
        m = ens.add(load_cfg("default.soil"), 32, 32, seed=1, pool=1 << 14)
        L.smx_destroy(m.h)
        assert b"ensemble" in L.smx_last_error(m.h)
        ens.tick(50, 0, dowind=False)
        ens.sync()
        assert m.counters()["steps_water_top"] > 0            # still alive; freed once, by the ensemble


# ---------------------------------------------------------------- 5. one launch shape for any size
def _launches(nmembers: int) -> dict:
    cfg = load_cfg("rockgravelpebblessand.soil")
    with Ensemble(0) as ens:
        for s in range(nmembers):
            ens.add(cfg, 32, 32, seed=s, pool=1 << 15)
        ens.tick(20, 10)
        ens.timing_reset()
        ens.tick(20, 10)
        t = ens.timing()
    return {k: v for k, v in t.items() if k.startswith("launches")}


def test_launch_count_does_not_depend_on_member_count():
    two, many = _launches(2), _launches(64)
    assert two == many
    assert two["launches_kernel_water"] == 1 and two["launches_kernel_wind"] == 1
    assert two["launches_kernel_classify"] == 1 and two["launches_kernel_mapfreq"] == 1


# ---------------------------------------------------------------- 6. refusals and isolation
def test_refusals_leave_the_ensemble_working():
    L = capi.load()
    cfg = load_cfg("default.soil")
    with Ensemble(0) as ens:
        m = ens.add(cfg, 32, 32, seed=2, pool=1 << 14)
        for engine in (capi.ENGINE_SPECULATIVE, capi.ENGINE_BATCHED, capi.ENGINE_RELAXED):
            c = capi.Config(32, 32, cfg.SCALE, 0, 1 << 14, engine, 0)
            h = C.c_void_p()
            assert L.smx_ensemble_add(ens.h, C.byref(c), C.byref(h)) == -2
            assert not h and b"SERIAL" in L.smx_ensemble_last_error(ens.h)
        # (a strip context cannot be a member: smx_ensemble_add creates every member itself, always over the whole map)
        with pytest.raises(SoilmxError):
            ens.add(cfg, 0, 32, seed=0)                         # invalid dims: refused by the context's own checks
        with pytest.raises(SoilmxError, match="pool_capacity"):
            ens.add(cfg, 32, 32, seed=0, pool=32 * 32 - 1)      # added, then smx_initialize refuses the pool (-4): taken out again
        assert len(ens) == ens.size() == 1
        w = (C.c_int32 * 1)(10)
        assert L.smx_ensemble_tick(ens.h, None, w, 1, 1) == -2 and L.smx_ensemble_last_error(ens.h)
        assert L.smx_ensemble_tick(ens.h, w, None, 1, 1) == -2 and L.smx_ensemble_last_error(ens.h)
        assert L.smx_set_engine(m.h, capi.ENGINE_BATCHED) == 0  # a member switched off the exact engine stops the tick
        assert L.smx_ensemble_tick(ens.h, w, w, 1, 1) == -2 and b"SERIAL" in L.smx_ensemble_last_error(ens.h)
        assert L.smx_set_engine(m.h, capi.ENGINE_SERIAL) == 0
        with pytest.raises(ValueError):
            ens.tick([10, 10], 5)
        assert ens.size() == 1
        ens.tick(40, 10)
        ens.tick(30, None, dowind=False)                        # without wind nwind is not read: None does not make anyone sit out
        ens.sync()
        ref = Layermap(cfg, 32, 32, seed=2, pool=1 << 14)
        standalone_tick(ref, 40, 10, 1, 1)
        standalone_tick(ref, 30, 0, 1, 0)
        assert_same(m, ref, "member after the refused calls")
        ref.close()


def test_remove_a_member():
    cfg = load_cfg("rockgravelpebblessand.soil")
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, 32, 32, seed=s, pool=1 << 15) for s in range(3)]
        ens.tick(40, 10)
        ens.remove(mem[1])
        assert len(ens) == ens.size() == 2 and mem[1].h is None
        assert capi.load().smx_ensemble_remove(ens.h, mem[0].h) == 0
        ens.members.remove(mem[0])
        assert capi.load().smx_ensemble_remove(ens.h, mem[0].h) == -2   # (no longer a member: refused, nothing freed twice)
        mem[0].h = None
        ens.tick([40], [10])                                    # the remaining member keeps its place and its state
        ens.sync()
        ref = Layermap(cfg, 32, 32, seed=2, pool=1 << 15)
        for _ in range(2):
            standalone_tick(ref, 40, 10, 1, 1)
        assert_same(mem[2], ref, "member 2 after the removals")
        ref.close()


def test_pool_overflow_stays_with_its_member():
    cfg = load_cfg("rockgravelpebblessand.soil")                # (its sediment piles up in new sections: rgps64 ends with ~30 per cell)
    tiny = 64 * 64 * len(layers_array(cfg))                     # the least smx_initialize accepts: the sediment of the ticks does not fit
    specs = [("default.soil", 0, 1 << 18), ("rockgravelpebblessand.soil", 0, tiny), ("rockgravelpebblessand.soil", 5, 1 << 18)]
    with Ensemble(0) as ens:
        mem = [ens.add(load_cfg(s), 64, 64, seed=seed, pool=p) for s, seed, p in specs]
        ref = [Layermap(load_cfg(s), 64, 64, seed=seed, pool=p) for s, seed, p in specs]
        for _ in range(5):
            ens.tick(150, 40)
            for r in ref:
                standalone_tick(r, 150, 40, 1, 1)
        ens.sync()
        assert mem[1].counters()["pool_overflow"] > 0
        for i in range(3):
            assert_same(mem[i], ref[i], f"member {i}")          # the overflowing member as standalone, its neighbours untouched
        assert mem[0].counters()["pool_overflow"] == 0 and mem[2].counters()["pool_overflow"] == 0
        for r in ref:
            r.close()


# ---------------------------------------------------------------- 7. the measurement's workload, 256 members
@pytest.mark.slow
def test_256_members_of_the_default_workload():
    cfg = load_cfg("default.soil")
    n, ticks, nwater = 256, 20, 250
    pool = 8 * n * n
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, n, n, seed=s, pool=pool) for s in range(256)]
        ens.tick(nwater, 0, dowind=False, n=ticks)
        ens.sync()
        d = DIG["default256_t20"]
        s = mem[0].snapshot()
        g = s.digest()
        assert (g["nsec"], g["typehash"], g["sumh"], s.rand_calls) == (d["nsec"], d["typehash"], d["sumh"], d["rand_calls"])
        assert mem[0].counters()["steps_water_top"] == d["steps_water_top"]
        for i in (1, 17, 64, 101, 128, 170, 203, 255):
            ref = Layermap(cfg, n, n, seed=i, pool=pool)
            for _ in range(ticks):
                standalone_tick(ref, nwater, 0, 1, 0)
            assert_same(mem[i], ref, f"member {i}")
            ref.close()
        assert all(m.counters()["pool_overflow"] == 0 for m in mem)
