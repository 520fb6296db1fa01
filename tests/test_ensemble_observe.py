"""An ensemble observed as one thing (smx_ensemble_figures / smx_ensemble_plane_stats) without a GPU: the entry points, and the
bodies of k_ens_figures / k_ens_plane_stats (soilmachine_amd/csrc/soil_observe.h) compiled for the host by tests/observe_host and
run with the lanes looped, against numpy on the committed golden snapshots and on a synthetic map."""
import ctypes as C

import numpy as np
import pytest

from common import SNAP_CASES, digests, golden_snapshot
from observe_host_lib import NIL, VARIANTS, HostMember, plane_stats
from observe_ref import f64_bits, figures_ref, same_bits, stats_ref, water_plane
from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

DIG = digests()
SNAPS = [(case, t) for case in SNAP_CASES for t in SNAP_CASES[case][3]]
KERNEL_K = VARIANTS[0][1]                    # buried types per cell the kernel's own shape stages
SHAPES = [(lanes, v) for v in VARIANTS for lanes in (64, 256)] + [(128, 0), (192, 1)]


def assert_figures(got: dict, want: dict, what):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float):
            assert f64_bits(g) == f64_bits(w), f"{what}: {k} = {g!r}, expected {w!r}"
        else:
            assert g == w, f"{what}: {k} = {g!r}, expected {w!r}"


# ---------------------------------------------------------------- 1. symbols, struct size, refusals without a device
def test_symbols_struct_size_and_refusals():
    L = capi.load()
    for n in ("smx_ensemble_figures", "smx_ensemble_plane_stats"):
        assert hasattr(L, n), f"libsoilmx.so does not export {n}"
        assert n in capi.SYMBOLS
    assert C.sizeof(capi.MemberFigures) == 80
    assert [n for n, _ in capi.MemberFigures._fields_] == ["sumh", "nsec", "typehash", "wet_cells", "water_volume", "hmin", "hmax", "empty_cells",
                                                           "rand_calls", "live_sections"]
    out = (capi.MemberFigures * 2)()
    mean = np.zeros(16)
    # NULL: refused, and the error reader has a text for it
    assert L.smx_ensemble_figures(None, out, 80) == -2
    assert L.smx_ensemble_plane_stats(None, 0, None, 0, capi.ptr(mean), None, None, None, None) == -2
    assert L.smx_ensemble_last_error(None)
    h = C.c_void_p()
    rc = L.smx_ensemble_create(0, C.byref(h))
    try:
        if rc != 0:        # no device: the handle of the failed create refuses both calls with a text
            assert L.smx_ensemble_figures(h, out, 80) != 0
            assert b"smx_ensemble_figures" in L.smx_ensemble_last_error(h)
            assert L.smx_ensemble_plane_stats(h, 0, None, 0, capi.ptr(mean), None, None, None, None) != 0
            assert b"smx_ensemble_plane_stats" in L.smx_ensemble_last_error(h)
        else:              # a device: an empty ensemble has no figures to write and no member to select
            assert L.smx_ensemble_figures(h, out, 80) == 0
            assert L.smx_ensemble_plane_stats(h, 0, None, 0, capi.ptr(mean), None, None, None, None) == -2
            assert L.smx_ensemble_last_error(h)
    finally:
        L.smx_ensemble_destroy(h)


# ---------------------------------------------------------------- 2. figures on every committed golden snapshot
@pytest.mark.parametrize("case,tick", SNAPS)
def test_figures_on_golden_snapshots(case, tick):
    s = golden_snapshot(case, tick)
    want = figures_ref(s)                       # sumh / nsec / typehash: Snapshot.digest(); the water fields: numpy
    want["rand_calls"] = int(s.rand_calls)
    want["live_sections"] = int(s.nsec)
    if DIG[case]["ticks"] == tick:              # ... and the reference's own recorded digest
        d = DIG[case]
        assert (want["nsec"], want["typehash"], f64_bits(want["sumh"])) == (d["nsec"], d["typehash"], f64_bits(d["sumh"]))
    m = HostMember(s)
    first = None
    for lanes, variant in SHAPES:
        rc, got = m.figures(lanes, variant)
        assert rc == 0 and got["corrupt"] == 0
        assert_figures(got, want, f"{case} t{tick}, {lanes} lanes, tile/staged {VARIANTS[variant]}")
        first = first or got
        assert got == first                    # identical whatever the width, the tile and the staging budget


def test_goldens_give_the_figures_real_ground():
    wet, longest = {}, {}
    for case, tick in SNAPS:
        m = HostMember(golden_snapshot(case, tick))
        rc, f = m.figures()
        assert rc == 0
        wet[(case, tick)] = f["wet_cells"]
        longest[(case, tick)] = m.longest_column()
    assert (wet[("default64", 5)], wet[("default64", 20)], wet[("default64s7", 40)]) == (261, 399, 36)
    assert any(w > 0 for w in wet.values())
    assert any(n - 1 > KERNEL_K for n in longest.values())      # buried sections beyond the staged ones: the overflow path runs
    assert max(longest.values()) == 893


# ---------------------------------------------------------------- 3. a synthetic map: empty columns, water tops, odd dims
def synthetic(dimx=37, dimy=53, seed=5) -> Snapshot:
    rng = np.random.default_rng(seed)
    nc = dimx * dimy
    count = rng.integers(1, 41, nc).astype(np.uint32)
    count[rng.random(nc) < 0.12] = 0
    ty, size, floor = [], [], []
    for c in range(nc):
        k = int(count[c])
        t = rng.integers(1, 7, k).astype(np.uint32)
        if k and rng.random() < 1 / 3:
            t[-1] = 0                                            # water on top
        if k > 2 and rng.random() < 0.2:
            t[rng.integers(0, k - 1)] = 0                        # ... and buried Air, which is no standing water
        sz = rng.random(k) * 0.05 + 1e-4
        fl = np.concatenate(([0.0], np.cumsum(sz)[:-1])) if k else np.zeros(0)
        ty.append(t); size.append(sz); floor.append(fl)
    ty = np.concatenate(ty).astype(np.uint32); size = np.concatenate(size); floor = np.concatenate(floor)
    f = rng.random(nc).astype(np.float32)
    return Snapshot(dimx, dimy, 80, 7, 12345, 0, count, ty, size, floor, np.zeros_like(size), f, np.zeros(nc, np.float32), (f * 3).astype(np.float32))


def test_figures_on_a_synthetic_map():
    s = synthetic()
    want = figures_ref(s)
    want["rand_calls"], want["live_sections"] = 12345, int(s.nsec)
    assert want["empty_cells"] > 50 and want["wet_cells"] > 300 and want["hmin"] == 0.0 and int(s.count.max()) == 40
    m = HostMember(s, pool=s.nsec + 17)
    for lanes, variant in SHAPES:
        rc, got = m.figures(lanes, variant)
        assert rc == 0
        assert_figures(got, want, f"synthetic, {lanes} lanes, tile/staged {VARIANTS[variant]}")


# ---------------------------------------------------------------- 4. plane statistics over the 64 x 64 golden snapshots
def snaps64():
    out = [golden_snapshot(c, t) for c, t in SNAPS]
    return [s for s in out if (s.dimx, s.dimy) == (64, 64)]


def test_plane_stats_bodies_equal_the_numpy_member_loop():
    snaps = snaps64()
    assert len(snaps) >= 9
    mem = [HostMember(s) for s in snaps]
    n = len(mem)
    orders = [list(range(n)), [int(i) for i in np.random.default_rng(1).permutation(n)]]
    assert sorted(orders[1]) == orders[0] and orders[1] != orders[0]
    planes = {"height": [s.heights() for s in snaps], "water": [water_plane(s) for s in snaps],
              "wfreq": [s.wfreq for s in snaps], "windfreq": [s.windfreq for s in snaps]}
    assert sum(int((w != 0).sum()) for w in planes["water"]) > 0
    for plane, vals in planes.items():
        res = []
        for order in orders:
            got = plane_stats([mem[i] for i in order], plane)
            want = stats_ref([vals[i] for i in order])
            for k in ("mean", "var", "vmin", "vmax", "nonzero"):
                assert same_bits(got[k], want[k]), f"{plane}: {k} differs from the numpy loop (order {order})"
            novar = plane_stats([mem[i] for i in order], plane, var=False)
            assert "var" not in novar and all(same_bits(novar[k], got[k]) for k in novar)
            res.append(got)
        a, b = res
        # another order: the extremes and the count are the same values; the sums may differ by what f64 addition allows -- each
        # sequential sum of n terms is within (n-1) eps sum|v| of the exact one (Higham, Accuracy and Stability, eq. 4.4), the
        # division by n adds one rounding each
        for k in ("vmin", "vmax", "nonzero"):
            assert same_bits(a[k], b[k]), (plane, k)
        mean_abs = stats_ref([np.abs(np.asarray(v, np.float64)) for v in vals], var=False)["mean"]
        bound = 2 * n * np.finfo(np.float64).eps * mean_abs * (1 + 1e-9)
        assert np.all(np.abs(a["mean"] - b["mean"]) <= bound), plane
        # var: the two means differ by delta <= bound, so every d_i = v_i - mean moves by delta: sum((d - delta)^2)/n - sum(d^2)/n =
        # -2 delta mean(d) + delta^2 with |mean(d)| <= sqrt(var); on top, each d_i and d_i^2 is rounded (3 eps relative) and each
        # sequential sum of the n squares is within (n-1) eps of its exact value, the division adds one rounding: (n+3) eps var each
        eps = np.finfo(np.float64).eps
        vmax_ = np.maximum(a["var"], b["var"])
        vbound = (2 * (n + 3) * eps * vmax_ + 2 * bound * np.sqrt(vmax_) + bound * bound) * (1 + 1e-9)
        assert np.all(np.abs(a["var"] - b["var"]) <= vbound), plane
    one = plane_stats([mem[3]], "height")
    assert same_bits(one["mean"], snaps[3].heights()) and not one["var"].any()
    assert same_bits(one["vmin"], one["mean"]) and same_bits(one["vmax"], one["mean"])


# ---------------------------------------------------------------- 5. a corrupt chain ends with -5, not with a hang
def test_corrupt_chain_is_reported():
    s = golden_snapshot("rgps64", 3)
    cell = int(np.argmax(s.count))
    for variant in VARIANTS:
        m = HostMember(s)
        p = int(m.L.oh_top_prev(m.h, cell))
        assert p != NIL
        m.L.oh_set_prev(m.h, cell, p, p)                         # the first buried section is its own predecessor
        rc, got = m.figures(256, variant)
        assert rc == -5 and got["corrupt"] == 1
        m.L.oh_set_prev(m.h, cell, NIL, m.pool + 5)              # the top's link leaves the pool
        rc, got = m.figures(64, variant)
        assert rc == -5 and got["corrupt"] == 1
