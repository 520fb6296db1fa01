"""An ensemble observed as one thing on a real MI355X (smx_ensemble_figures / smx_ensemble_plane_stats, k_ens_figures /
k_ens_plane_stats): every number bit-identical to the per-member readers on the same state and to the reference's digests."""
import ctypes as C

import numpy as np
import pytest

from common import digests, load_cfg
from observe_ref import f64_bits, figures_ref, same_bits, stats_ref, water_plane
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap, SoilmxError
from soilmachine_amd.snapshot import compare
from test_gpu_ensemble import DIGEST_MEMBERS, assert_same, digest_case, rand_state, standalone_tick

pytestmark = pytest.mark.gpu
DIG = digests()
FLOATS = ("sumh", "water_volume", "hmin", "hmax")


def per_member(m) -> dict:
    """The same numbers through the per-member entry points: smx_digest, the generator and counter getters, exported columns."""
    d = m.digest()
    ns = C.c_uint64()
    m._chk(m.L.smx_num_sections(m.h, C.byref(ns)))
    out = figures_ref(m.snapshot())
    assert (out["nsec"], out["typehash"], f64_bits(out["sumh"])) == (d["nsec"], d["typehash"], f64_bits(d["sumh"]))
    out["rand_calls"] = rand_state(m)[2]
    out["live_sections"] = int(ns.value)
    return out


def assert_figures(got: dict, want: dict, what):
    assert set(got) == set(want), what
    for k, w in want.items():
        if k in FLOATS:
            assert f64_bits(got[k]) == f64_bits(w), f"{what}: {k} = {got[k]!r}, expected {w!r}"
        else:
            assert got[k] == w, f"{what}: {k} = {got[k]!r}, expected {w!r}"


# ---------------------------------------------------------------- 1. the reference's digests, mixed members, one call
def test_figures_reproduce_reference_digests():
    with Ensemble(0) as ens:
        runs = []
        for case in DIGEST_MEMBERS:
            cfg, dimx, dimy, seed, nwater, nwind, ticks = digest_case(case)
            runs.append((case, ens.add(cfg, dimx, dimy, seed=seed), nwater, nwind, ticks))
        for t in range(max(r[4] for r in runs)):
            ens.tick([nw if t < tk else None for _, _, nw, _, tk in runs], [nd for _, _, _, nd, _ in runs])
        figs = ens.figures()                                    # (no sync: the call is queued behind the ticks)
        assert len(figs) == len(runs)
        for (case, m, _, _, _), f in zip(runs, figs):
            d = DIG[case]
            assert (f["nsec"], f["typehash"], f64_bits(f["sumh"]), f["rand_calls"]) == (d["nsec"], d["typehash"], f64_bits(d["sumh"]), d["rand_calls"]), case
            g = m.digest()
            assert (f["nsec"], f["typehash"], f64_bits(f["sumh"]), f["rand_calls"]) == (g["nsec"], g["typehash"], f64_bits(g["sumh"]), g["rand_calls"]), case
            assert f["live_sections"] == f["nsec"], case


# ---------------------------------------------------------------- 2. queued ticks are seen without a sync
def test_figures_see_queued_ticks():
    cfgs = [load_cfg("default.soil"), load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")]
    with Ensemble(0) as ens:
        mem = [ens.add(cfgs[0], 64, 64, seed=4, pool=1 << 18), ens.add(cfgs[1], 64, 64, seed=1, pool=1 << 19), ens.add(cfgs[2], 33, 47, seed=7, pool=1 << 18)]
        ens.tick([120, 90, 60], [0, 40, 30], n=4)
        figs = ens.figures()                                    # right behind the ticks
        heights = ens.plane_stats("height", [1])["mean"]
        ens.sync()
        for i, m in enumerate(mem):
            assert_figures(figs[i], per_member(m), f"member {i}")
        assert same_bits(heights, mem[1].heights())
        assert figs[1]["nsec"] > 64 * 64


# ---------------------------------------------------------------- 3. the water fields on the device
def test_water_fields_on_the_device():
    with Ensemble(0) as ens:
        a = ens.add(load_cfg("default.soil"), 64, 64, seed=0, pool=1 << 18)
        b = ens.add(load_cfg("rockgravelpebblessand.soil"), 48, 80, seed=2, pool=1 << 19)
        ens.tick([150, 80], [0, 40], n=3)
        ens.sync()
        for k, (x, y) in enumerate([(3, 4), (3, 5), (17, 40), (63, 63), (0, 0), (31, 32), (40, 9)]):
            a.add(x, y, 0.004 + 0.0011 * k, 0)                  # standing water, whether or not a lake has formed by itself
        b.add(5, 70, 0.02, 0)
        figs = ens.figures()
        for i, m in enumerate((a, b)):
            assert_figures(figs[i], per_member(m), f"member {i}")
        assert figs[0]["wet_cells"] >= 7 and figs[1]["wet_cells"] >= 1 and figs[0]["water_volume"] > 0.0
        assert figs[1]["nsec"] > 48 * 80
        w = ens.plane_stats("water", [a])
        assert same_bits(w["mean"], water_plane(a.snapshot())) and int(w["nonzero"].sum()) == figs[0]["wet_cells"]


# ---------------------------------------------------------------- 4. cross-member statistics of every plane
def member_planes(m) -> dict:
    wf, _, wi = m.frequency()
    return {"height": m.heights(), "water": water_plane(m.snapshot()), "wfreq": wf, "windfreq": wi}


def test_plane_stats_equal_the_numpy_member_loop():
    rgps, rocksand = load_cfg("rockgravelpebblessand.soil"), load_cfg("rocksand.soil")
    with Ensemble(0) as ens:
        mem = [ens.add(rgps, 64, 64, seed=s, pool=64 * 64 * 64) for s in range(33)]
        odd = ens.add(rocksand, 33, 47, seed=7, pool=64 * 33 * 47)
        ens.tick([60 + 5 * (i % 7) for i in range(34)], [20 + 3 * (i % 5) for i in range(34)], n=6)
        for i, x, y, size in ((4, 10, 10, 0.01), (9, 10, 10, 0.02), (9, 50, 3, 0.005), (30, 63, 0, 0.03)):
            mem[i].add(x, y, size, 0)                           # water in some runs, whether or not a lake has formed by itself
        planes = [member_planes(m) for m in mem]
        subset = [int(i) for i in np.random.default_rng(3).permutation(33)[:7]]
        for plane in ("height", "water", "wfreq", "windfreq"):
            for sel in (list(range(33)), subset):
                got = ens.plane_stats(plane, sel)
                want = stats_ref([planes[i][plane] for i in sel])
                assert set(got) == set(want)
                for k in want:
                    assert got[k].shape == (64 * 64,) and same_bits(got[k], want[k]), f"{plane}, members {sel}: {k}"
                lean = ens.plane_stats(plane, [mem[i] for i in sel], var=False, minmax=False, nonzero=False)
                assert set(lean) == {"mean"} and same_bits(lean["mean"], want["mean"])
            assert any(p[plane].any() for p in planes), plane   # (no plane is trivially zero: wind and water have run)
        alone = ens.plane_stats("height", [odd])
        assert same_bits(alone["mean"], odd.heights()) and not alone["var"].any()
        with pytest.raises(SoilmxError, match=r"member 33 is 33x47"):
            ens.plane_stats("height", [mem[2], odd])
        with pytest.raises(SoilmxError, match=r"member 33 is 33x47"):
            ens.plane_stats("wfreq")                          # all members: the odd one is named
        with pytest.raises(SoilmxError, match="no member selected"):
            ens.plane_stats("height", [])
        with pytest.raises(SoilmxError, match="member 5 is selected twice"):
            ens.plane_stats("height", [1, 5, 9, 5])
        with pytest.raises(SoilmxError, match=r"which\[1\] = 34"):
            ens.plane_stats("height", [0, 34])
        with pytest.raises(SoilmxError, match=r"which\[0\] = -1"):
            ens.plane_stats("height", [-1])
        w = np.zeros(4, np.int32)                             # more indices than members: refused before anything is sized by n
        assert ens.L.smx_ensemble_plane_stats(ens.h, 0, capi.ptr(w), 2**31 - 1, None, None, None, None, None) == -2
        assert "2147483647" in ens.last_error()
        ens.remove(odd)                                       # which == NULL: all members in member order, n ignored
        mean = np.zeros(64 * 64)
        assert ens.L.smx_ensemble_plane_stats(ens.h, 0, None, -7, capi.ptr(mean), None, None, None, None) == 0
        assert same_bits(mean, stats_ref([p["height"] for p in planes])["mean"])


# ---------------------------------------------------------------- 5. remove and sit-out
def test_figures_after_remove_and_sit_out():
    cfg = load_cfg("rockgravelpebblessand.soil")
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, 32, 32, seed=s, pool=1 << 15) for s in range(4)]
        ens.tick(40, 10)
        before = ens.figures()
        ens.tick([40, None, 40, 40], 10)                        # member 1 sits this tick out
        after = ens.figures()
        assert after[1] == before[1]
        assert all(after[i] != before[i] for i in (0, 2, 3))
        ens.remove(mem[1])
        figs = ens.figures()
        assert len(figs) == 3 and figs == [after[0], after[2], after[3]]
        for f, m in zip(figs, (mem[0], mem[2], mem[3])):
            assert_figures(f, per_member(m), "after the removal")
        st = ens.plane_stats("height")
        assert same_bits(st["mean"], stats_ref([m.heights() for m in (mem[0], mem[2], mem[3])])["mean"])


# ---------------------------------------------------------------- 6. observing changes nothing
def test_observing_has_no_side_effects():
    rgps, dflt = load_cfg("rockgravelpebblessand.soil"), load_cfg("default.soil")
    specs = [(rgps, 64, 64, 0), (dflt, 64, 64, 3), (rgps, 64, 64, 5), (dflt, 64, 64, 8)]
    nwater, nwind = [80, 120, 70, 100], [30, 0, 25, 10]
    with Ensemble(0) as ens:
        mem = [ens.add(cfg, dx, dy, seed=s, pool=1 << 19) for cfg, dx, dy, s in specs]
        ref = [Layermap(cfg, dx, dy, seed=s, pool=1 << 19) for cfg, dx, dy, s in specs]
        try:
            ens.tick(nwater, nwind, n=3)
            for i, r in enumerate(ref):
                for _ in range(3):
                    standalone_tick(r, nwater[i], nwind[i], 1, 1)
            ens.sync()
            state = [(m.snapshot(), rand_state(m), m.counters()) for m in mem]
            figs = ens.figures()
            for plane in ("height", "water", "wfreq", "windfreq"):
                ens.plane_stats(plane)
            assert ens.figures() == figs
            for m, (s, r, c) in zip(mem, state):
                assert not compare(m.snapshot(), s) and rand_state(m) == r and m.counters() == c
            ens.tick(nwater, nwind, n=3)
            for i, r in enumerate(ref):
                for _ in range(3):
                    standalone_tick(r, nwater[i], nwind[i], 1, 1)
            ens.sync()
            for i in range(len(specs)):
                assert_same(mem[i], ref[i], f"member {i}, three ticks after the observation")
        finally:
            for r in ref:
                r.close()


# ---------------------------------------------------------------- 7. a caller with a shorter struct gets its prefix
def test_struct_size_prefix():
    L = capi.load()
    with Ensemble(0) as ens:
        for s in range(3):
            ens.add(load_cfg("default.soil"), 32, 32, seed=s, pool=1 << 14)
        full = ens.figures()
        buf = np.full(3 * 3, 0xABABABABABABABAB, np.uint64)   # a caller whose struct ends after typehash: 24 bytes per entry
        assert L.smx_ensemble_figures(ens.h, capi.ptr(buf), 24) == 0
        for i, f in enumerate(full):
            assert int(buf[3 * i]) == f64_bits(f["sumh"]) and int(buf[3 * i + 1]) == f["nsec"] and f"{int(buf[3 * i + 2]):016x}" == f["typehash"]
