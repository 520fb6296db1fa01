"""Forking a spun-up map on a real MI355X (smx_copy_state / smx_ensemble_fork; k_fork_count, k_fork_scatter, k_fork_planes): the
branches continue bit-identically -- to the reference's golden states, to save + load, to standalone contexts."""
import numpy as np
import pytest

from common import SNAP_CASES, case_dims, digests, golden_snapshot, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilmxError
from soilmachine_amd.snapshot import compare
from test_gpu_ensemble import rand_state, standalone_tick
from test_gpu_ensemble_observe import assert_figures, per_member

pytestmark = pytest.mark.gpu
DIG = digests()
COLUMNS = ("count", "type", "size", "floor", "sat")


def golden_source(case, tick, pool=1 << 18):
    """A standalone SERIAL context driven as the golden case is, ticked to `tick`: (map, nwater, nwind)."""
    soil, seed, dowind, _ = SNAP_CASES[case]
    cfg = load_cfg(soil)
    d = DIG[case]
    dimx, dimy = case_dims(d, cfg)
    nwater, nwind = d["nwater"], d["nwind"] if dowind else 0
    m = Layermap(cfg, dimx, dimy, seed=seed, pool=pool)
    for _ in range(tick):
        standalone_tick(m, nwater, nwind, 1, 1)
    return m, nwater, nwind


def same_columns(a, b) -> bool:
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in COLUMNS)


def state(m):
    return m.digest(), m.counters()


# ---------------------------------------------------------------- 1. pinned to the reference's goldens
# rgps64: a pool of exactly the section count of the golden tick 10 (124 893) overflows -- 12 pool.get() failures on the device and
# in the CPU oracle alike: within a tick the map briefly holds one section more than at its end. 124 894 is the smallest pool that does
# not overflow (bisected with the CPU oracle, which reaches the golden tick 10 with it and misses it with 124 893), so the members get that.
RGPS64_POOL = 124894
@pytest.mark.parametrize("case,t0,t1,pool", [("default64", 5, 20, 8 * 64 * 64), ("rgps64", 3, 10, RGPS64_POOL)])
def test_forked_members_reach_the_golden_states(case, t0, t1, pool):
    src, nwater, nwind = golden_source(case, t0)
    try:
        assert not compare(src.snapshot(), golden_snapshot(case, t0))
        with Ensemble(0) as ens:
            mem = ens.fork(src, 3, pool=pool)
            assert len(mem) == 3 and ens.size() == 3 and all(m.pool == pool and (m.dimx, m.dimy) == (src.dimx, src.dimy) for m in mem)
            for m in mem:
                assert rand_state(m) == rand_state(src)
            ens.tick(nwater, nwind, n=t1 - t0)
            for _ in range(t1 - t0):
                standalone_tick(src, nwater, nwind, 1, 1)
            ens.sync()
            want = golden_snapshot(case, t1)
            for i, m in enumerate(mem):
                c = m.counters()
                print(f"{case}: member {i} pool {pool}, pool_free {c['pool_free']}, pool_overflow {c['pool_overflow']}")
                assert c["pool_overflow"] == 0, f"{case}: member {i} ran out of its {pool} sections"
                bad = compare(m.snapshot(), want)
                assert not bad, f"{case} member {i} at tick {t1}: {bad}"
                assert rand_state(m) == rand_state(src), f"{case} member {i}: rand() generator"
    finally:
        src.close()


# ---------------------------------------------------------------- 2. copy_state == save + load, every engine
@pytest.mark.parametrize("engine", [capi.ENGINE_SERIAL, capi.ENGINE_SPECULATIVE, capi.ENGINE_BATCHED, capi.ENGINE_RELAXED],
                         ids=["serial", "speculative", "batched", "relaxed"])
def test_copy_state_equals_save_and_load(engine, tmp_path):
    cfg = load_cfg("default.soil")
    nwater, nwind = 250, 60
    src = Layermap(cfg, 64, 64, seed=0, pool=1 << 18, engine=engine)
    dst_a = Layermap(cfg, 64, 64, seed=5, pool=3 * 64 * 64, engine=engine)                          # another terrain, another pool size
    dst_b = Layermap(cfg, 64, 64, seed=7, pool=3 * 64 * 64, engine=engine)
    ms = (src, dst_a, dst_b)
    try:
        for _ in range(6):
            standalone_tick(src, nwater, nwind, 1, 1)
        standalone_tick(dst_a, 40, 10, 1, 1)                    # (a used destination: counters, planes, a pool in disorder)
        before = dst_a.counters()
        dst_a.copy_from(src)
        path = str(tmp_path / "src.smx")
        src.save(path)
        assert dst_b.restore(path)
        after = dst_a.counters()
        for k, v in before.items():                             # dst's other counters stay as they are
            if k not in ("rand_calls", "pool_free"):
                assert after[k] == v, k
        assert not compare(dst_a.snapshot(), src.snapshot()) and rand_state(dst_a) == rand_state(src)
        assert not compare(dst_a.snapshot(), dst_b.snapshot())
        for _ in range(4):
            for m in ms:
                standalone_tick(m, nwater, nwind, 1, 1)
        sa, sb, ss = dst_a.snapshot(), dst_b.snapshot(), src.snapshot()
        assert not compare(sa, sb), compare(sa, sb)
        assert rand_state(dst_a) == rand_state(dst_b)
        assert dst_a.counters()["pool_free"] == dst_b.counters()["pool_free"]
        assert same_columns(sa, ss) and same_columns(sb, ss), "the copies left the source's trajectory"
        assert dst_a.counters()["pool_overflow"] == before["pool_overflow"] and dst_b.counters()["pool_overflow"] == 0
    finally:
        for m in ms:
            m.close()


# ---------------------------------------------------------------- 3. seeds
def test_seeded_members_equal_reseeded_standalone_contexts():
    seeds = [11, 12, 13, 14]
    src, nwater, nwind = golden_source("rgps64", 3)
    ref = []
    try:
        snap = src.snapshot()
        with Ensemble(0) as ens:
            mem = ens.fork(src, 4, seeds=seeds, pool=1 << 18)
            ens.tick(nwater, nwind, n=5)
            for sd in seeds:
                r = Layermap(src.cfg, src.dimx, src.dimy, seed=0, pool=1 << 18, initialize=False)
                ref.append(r)
                r.load(snap)
                r._chk(r.L.smx_srand(r.h, sd))
                for _ in range(5):
                    standalone_tick(r, nwater, nwind, 1, 1)
            ens.sync()
            for i, (m, r) in enumerate(zip(mem, ref)):
                bad = compare(m.snapshot(), r.snapshot())
                assert not bad, f"seed {seeds[i]}: {bad}"
                assert rand_state(m) == rand_state(r), f"seed {seeds[i]}: rand() generator"
            assert len({rand_state(m) for m in mem}) == 4
        assert not compare(src.snapshot(), snap), "the source was written"
    finally:
        src.close()
        for r in ref:
            r.close()


# ---------------------------------------------------------------- 4. sources: members of this and another ensemble, other dims
def test_fork_from_members_and_into_a_mixed_ensemble():
    rgps, dflt = load_cfg("rockgravelpebblessand.soil"), load_cfg("default.soil")
    odd, nw_odd, nd_odd = golden_source("rocksand48x80", 2)
    try:
        with Ensemble(0) as ens, Ensemble(0) as other:
            a = ens.add(rgps, 64, 64, seed=1, pool=1 << 18)
            b = ens.add(dflt, 64, 64, seed=2, pool=1 << 17)
            far = other.add(dflt, 64, 64, seed=3, pool=1 << 17)
            ens.tick([80, 120], [30, 0], n=2)
            other.tick(100, 20, n=2)                             # (queued on another stream: the fork must wait for it)
            fa = ens.fork(a, 2)                                  # a member of the same ensemble, right behind its ticks
            ff = ens.fork(far, 1, pool=1 << 16)                  # a member of another ensemble
            early = [a, b] + fa + ff
            was = [(m.snapshot(), m.counters(), rand_state(m)) for m in early]
            fo = ens.fork(odd, 2, seeds=[5, 6], pool=1 << 17)    # 48 x 80 into an ensemble of 64 x 64 members
            for m, (s, c, r) in zip(early, was):
                assert not compare(m.snapshot(), s) and m.counters() == c and rand_state(m) == r, "an earlier member changed"
            assert ens.size() == len(ens.members) == 7 and ens.members == early + fo
            assert [m.pool for m in ens.members] == [1 << 18, 1 << 17, 1 << 18, 1 << 18, 1 << 16, 1 << 17, 1 << 17]
            for m in fa:
                assert not compare(m.snapshot(), a.snapshot()) and rand_state(m) == rand_state(a)
                c = m.counters()
                assert all(v == 0 for k, v in c.items() if k not in ("rand_calls", "pool_free")), c
            assert not compare(ff[0].snapshot(), far.snapshot()) and rand_state(ff[0]) == rand_state(far)
            for m in fo:
                assert same_columns(m.snapshot(), odd.snapshot()) and (m.dimx, m.dimy) == (48, 80)
            figs = ens.figures()
            for i, m in enumerate(ens.members):
                assert_figures(figs[i], per_member(m), f"member {i}")
            ens.tick([80, 120, 80, 80, 100, nw_odd, nw_odd], [30, 0, 30, 30, 20, nd_odd, nd_odd], n=2)
            other.tick(100, 20, n=2)
            ens.sync(); other.sync()
            assert not compare(fa[0].snapshot(), a.snapshot()) and not compare(fa[1].snapshot(), a.snapshot())
            assert not compare(ff[0].snapshot(), far.snapshot())
            assert compare(fo[0].snapshot(), fo[1].snapshot()), "two seeds, one trajectory"
    finally:
        odd.close()


# ---------------------------------------------------------------- 5. many members in one call
def test_seventy_members_in_one_call():
    src, _, _ = golden_source("default64", 2, pool=1 << 16)
    try:
        with Ensemble(0) as ens:
            first = ens.add(src.cfg, 64, 64, seed=9, pool=1 << 15)     # (member 0 is no fork: the new ones are appended)
            mem = ens.fork(src, 70, pool=2 * 64 * 64)
            assert len(mem) == 70 and ens.size() == len(ens.members) == 71 and ens.members[0] is first
            want, rs = src.snapshot(), rand_state(src)
            for i, m in enumerate(mem):
                bad = compare(m.snapshot(), want)
                assert not bad, f"member {i}: {bad}"
                assert rand_state(m) == rs and m.counters()["pool_free"] == 2 * 64 * 64 - want.nsec
    finally:
        src.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_everything_as_it_was():
    cfg = load_cfg("default.soil")
    src = Layermap(cfg, 64, 64, seed=0, pool=1 << 16)
    small = Layermap(cfg, 48, 80, seed=0, pool=1 << 16)
    strip = Layermap(cfg, 64, 64, seed=0, pool=1 << 16, initialize=False, x_range=(0, 32))
    try:
        nsec = src.snapshot().nsec
        with Ensemble(0) as ens:
            ens.add(cfg, 64, 64, seed=1, pool=1 << 15)
            ens.fork(src, 2, pool=nsec)                            # (the pool that is one larger than the refused one succeeds)
            was = [state(m) for m in ens.members] + [state(src), state(small)]

            def unchanged():
                assert ens.size() == len(ens.members) == 3
                assert [state(m) for m in ens.members] + [state(src), state(small)] == was

            for kw, text in (({"src": strip}, "strip context"), ({"n": 0}, "n = 0"), ({"n": capi.ENSEMBLE_MAX_MEMBERS - 2}, "SMX_ENSEMBLE_MAX_MEMBERS"),
                             ({"pool": nsec - 1}, f"{nsec} live sections, more than the destination's pool_capacity {nsec - 1}")):
                with pytest.raises(SoilmxError, match=text) as ei:
                    ens.fork(kw.get("src", src), kw.get("n", 1), pool=kw.get("pool", 1 << 15))
                assert ("rc=-4" if "pool" in kw else "rc=-2") in str(ei.value)
                unchanged()
            with pytest.raises(SoilmxError, match="the dims must be equal"):
                small.copy_from(src)
            unchanged()
            with pytest.raises(SoilmxError, match="the same context"):
                src.copy_from(src)
            unchanged()
            with pytest.raises(SoilmxError, match="strip context"):
                src.copy_from(strip)
            unchanged()
            m = ens.members[1]
            with pytest.raises(SoilmxError, match=r"rc=-4"):     # a member's pool is too small for the source: the member stays as it was
                big, _, _ = golden_source("rgps64", 0, pool=1 << 18)
                try:
                    m.copy_from(big)
                finally:
                    big.close()
            unchanged()
            with pytest.raises(ValueError):
                ens.fork(src, 2, seeds=[1, 2, 3])
            unchanged()
    finally:
        for m in (src, small, strip):
            m.close()
