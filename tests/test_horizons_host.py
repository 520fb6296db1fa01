"""The horizon bodies (soil_horizon.h) compiled for the host (tests/horizons_host) against the plain-loop restatement
tests/horizons_ref.py: every plane, the sun counts and every record field, doubles by their bits -- in every tile shape, so that the
skips across fine and coarse tile edges are taken at small maps; the restatement's own invariants; the stand-alone sanitizer program;
the helpers of the Python binding and the refusals that need no device."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import drainage_ref as D
import horizons_ref as R
import lakes_ref as L
from horizons_host_lib import horizons as H, horizons_no_tiles as HN, build_check, run_check, write_columns
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # five pairs of tile sides, the kernels' own among them
WIDTHS = (64, 128, 256)
ALL16 = 0xFFFF
NAMES = sorted(D.INPUTS) + sorted(n for n in R.INPUTS if n not in D.INPUTS)
SMALL = [(33, 47), (1, 70), (70, 1)]


def test_the_shapes_and_the_constants():
    assert H.variants()[0] == (8, 64) and all(c >= f and f & (f - 1) == 0 and c & (c - 1) == 0 for f, c in H.variants().values())
    assert H.lib().hz_tiles_off() == 0 and HN.lib().hz_tiles_off() == 1
    assert (R.SQRT2, R.SQRT5) == (math.sqrt(2.0), math.sqrt(5.0))                       # the literals are the f64 nearest the roots
    assert capi.HORIZON_DIRECTIONS == R.DIRS and C.sizeof(capi.Horizon) == 64 and C.sizeof(capi.Sun) == 16
    az = [math.atan2(uy, ux) % (2 * math.pi) for ux, uy in R.DIRS]
    assert az == sorted(az), "the directions run counter-clockwise from +x"
    assert [R.LEN[d] ** 2 for d in (0, 4, 8, 12)] == [1.0] * 4 and all(R.LEN[d] == math.sqrt(sum(u * u for u in R.DIRS[d])) for d in range(16))


# ---------------------------------------------------------------- 1. every input at every size, every tile shape
@pytest.mark.parametrize("dims", L.SIZES, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("name", NAMES)
def test_inputs_equal_the_restatement(name, dims):
    for reach in R.REACHES:
        s, suns, want = R.case(name, dims, ALL16, reach)
        m = H.HostMap(s)
        for v in VARIANTS:                                     # (the widths and the orders go round with the shapes; all of them meet in the next test)
            got = H.run_many([m], ALL16, reach, suns, v, WIDTHS[(v + reach) % 3], (v + reach) % 4)[0]
            R.assert_same_horizons(got, want, f"{name} {dims} reach {reach} variant {v}")
        if dims in SMALL and reach != 1 and name != "extremes":   # (a subnormal slope is > 0 and its 1 / (1 + S*S) is 1.0: sky says open where open does not)
            R.assert_invariants(s, ALL16, reach, suns, *want, what=f"{name} {dims} reach {reach}")


@pytest.mark.parametrize("name,dims", [("random_bernoulli20", (33, 47)), ("integer_ties", (96, 80)), ("nan_inf", (64, 64))])
def test_every_shape_width_and_order(name, dims):
    s, suns, want = R.case(name, dims, ALL16, 0)
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in range(4):
                R.assert_same_horizons(H.run_many([m], ALL16, 0, suns, v, lanes, order)[0], want, f"{name} variant {v} lanes {lanes} order {order}")
    R.assert_same_horizons(HN.run_many([m], ALL16, 0, suns)[0], want, f"{name}: the scan without tile levels")


def test_the_skip_loads_fewer_heights_and_the_walk_all_of_them():
    s, suns, want = R.case("cone", (96, 80), ALL16, 0)
    walk, skip = HN.run(s, ALL16, 0, suns)[3], H.run(s, ALL16, 0, suns)[3]
    steps = sum(max(0, 96 - k * abs(ux)) * max(0, 80 - k * abs(uy)) for ux, uy in R.DIRS for k in range(1, 96))
    assert walk == (16 * 96 * 80, 0, steps), "without the levels a ray loads every cell on it"
    assert skip[0] == walk[0] and skip[2] < walk[2] and skip[1] > 0     # (a bowl: the horizon is the far rim, the skip saves least)
    s, suns, want = R.case("spike", (96, 80), ALL16, 0)
    walk, skip = HN.run(s, ALL16, 0, suns)[3], H.run(s, ALL16, 0, suns)[3]
    assert walk[2] == steps and skip[2] <= 8 * skip[0], "flat ground: a height is loaded only inside the spike's fine tile, 8 steps of a ray at most"


# ---------------------------------------------------------------- 2. masks, reaches, suns
@pytest.mark.parametrize("name", ["integer_ties", "random_checker"])
def test_single_directions_and_sub_masks(name):
    s, _, want = R.case(name, (33, 47), ALL16, 5)
    for d in range(16):
        got = H.run(s, 1 << d, 5, [(d, 0.25)], variant=d % 5)
        ref = R.horizons(s, 1 << d, 5, [(d, 0.25)])
        R.assert_same_horizons(got, (R.attach(ref[0], [(d, 0.25)], ref[2]), ref[1], ref[2]), f"{name}: direction {d} alone")
        assert np.array_equal(got[1]["step"][0], want[1]["step"][d]) and np.array_equal(got[1]["slope"][0].view(np.uint64), want[1]["slope"][d].view(np.uint64))
    for mask in (0x0101, 0x8001, 0xAAAA, 0x0FF0):
        ref = R.horizons(s, mask, 5)
        R.assert_same_horizons(H.run(s, mask, 5, variant=2), ref, f"{name}: mask {mask:#x}")
        R.assert_invariants(s, mask, 5, (), *ref, what=f"{name}: mask {mask:#x}")


def test_suns_on_the_horizon_equal_to_a_slope_and_overhead():
    s, _, full = R.case("integer_ties", (33, 47), ALL16, 0)
    slopes = full[1]["slope"]
    occurring = float(np.median(slopes[3][slopes[3] > 0]))     # a tangent that IS the horizon slope of many cells: they are lit (not S > tangent)
    suns = [(0, 0.0), (3, occurring), (3, 0.0), (9, 1.0e6), (15, occurring), (0, 0.5)]
    want = R.horizons(s, ALL16, 0, suns)
    assert want[2][3] == 33 * 47 and want[2][0] == int((slopes[0] == 0).sum()) < 33 * 47
    assert want[2][1] > want[2][2] and int((slopes[3] == occurring).sum()) > 10
    for v in VARIANTS:
        got = H.run(s, ALL16, 0, suns, variant=v, lanes=WIDTHS[v % 3], order=v % 4)
        R.assert_same_horizons(got, (R.attach(want[0], suns, want[2]), want[1], want[2]), f"suns, variant {v}")
        assert got[0][3]["lit_cells"] == [want[2][1], want[2][2]] and got[0][1]["lit_cells"] == []
    R.assert_invariants(s, ALL16, 0, suns, *want, what="suns")
    many = [(d % 16, 0.125 * (d % 7)) for d in range(64)]      # the most suns a call takes
    want = R.horizons(s, ALL16, 5, many)
    R.assert_same_horizons(H.run(s, ALL16, 5, many), (R.attach(want[0], many, want[2]), want[1], want[2]), "64 suns")


# ---------------------------------------------------------------- 3. what the special inputs are there for
def test_a_ramp_ties_at_every_step():
    s, _, want = R.case("ramp", (33, 47), ALL16, 0)
    K, S = want[1]["step"], want[1]["slope"]
    assert (K[0][:-1] == 1).all() and (K[0][-1] == 0).all() and (S[0][:-1] == 1.0).all()     # s_k = k / k: the smallest k has it
    assert not K[8].any() and not K[4].any() and not K[12].any()                              # downhill and along the contour: open
    assert want[0][0]["step_max"] == 1 and want[0][0]["bounded"] == 32 * 47 and want[0][0]["step_sum"] == 32 * 47 and want[0][0]["step_max_cell"] == 0
    assert want[0][8] == dict(want[0][8], bounded=0, step_max=0, step_max_cell=R.NONE, step_sum=0) and L.bits(want[0][8]["slope_max"]) == 0


def test_a_spike_is_seen_from_afar_and_a_wall_from_below():
    s, _, want = R.case("spike", (64, 64), ALL16, 0)
    K = want[1]["step"]
    px, py = 42, 21
    for d, (ux, uy) in enumerate(R.DIRS):
        on = np.argwhere(K[d] > 0)
        assert len(on) and all((x + int(K[d][x, y]) * ux, y + int(K[d][x, y]) * uy) == (px, py) for x, y in on), f"direction {d}"
        assert want[0][d]["step_max"] == max(k for k in range(1, 64) if 0 <= px - k * ux < 64 and 0 <= py - k * uy < 64)
    assert int((want[1]["sky"] < 1.0).sum()) == sum(r["bounded"] for r in want[0])            # no cell sees the spike twice
    _, _, want = R.case("wall", (96, 80), ALL16, 5)
    K, op = want[1]["step"], want[1]["open"]
    assert (op[48:] == ALL16).all() and (K[0][43:48] == np.arange(5, 0, -1)[:, None]).all() and not K[0][:43].any()


def test_a_lake_shows_its_surface_and_an_empty_column_is_ground_zero():
    s, _, want = R.case("bowl_lake", (64, 64), ALL16, 0)
    wet = D.heights(s)[0].reshape(64, 64)
    assert wet.sum() > 100 and all((want[1]["step"][d][wet] > 0).all() for d in range(16))
    inner = np.zeros((64, 64), bool); inner[30:35, 30:35] = True
    assert (wet[inner]).all() and all((want[1]["step"][d][inner] >= 5).all() for d in (0, 4, 8, 12)), "over the lake a ray sees the shore, not the next wet cell"
    s, _, want = R.case("empty", (33, 47), ALL16, 1)
    h = R.surface(s)
    assert (h.reshape(-1)[[0, 33 * 47 - 1]] == 0.0).all() and h[h != 0.0].min() >= 1.0
    assert want[1]["open"][0, 0] == 0xFFE0 and want[1]["open"][32, 46] == 0xE0FF      # open only where the first step leaves the map
    assert want[1]["step"][2][0, 0] == 1 and want[1]["slope"][2][0, 0] == h[1, 1] / R.SQRT2


# ---------------------------------------------------------------- 4. several maps, records only, a short struct
def test_maps_of_different_sizes_in_one_call():
    which = (("random_bernoulli20", (64, 64)), ("nan_inf", (33, 47)), ("ties", (1, 70)), ("spike", (70, 1)), ("integer_ties", (96, 80)))
    cases = [R.case(n, d, 0x5A5A, 5) for n, d in which]
    suns = cases[0][1]
    maps = [H.HostMap(c[0]) for c in cases]
    for v, lanes, order in ((0, 256, 0), (1, 64, 3), (2, 128, 1), (4, 64, 2)):
        got = H.run_many(maps, 0x5A5A, 5, suns, v, lanes, order)
        for i, (g, c) in enumerate(zip(got, cases)):
            R.assert_same_horizons(g, c[2], f"map {i} of five, variant {v}")
            R.assert_same_horizons(H.run_many([maps[i]], 0x5A5A, 5, suns, v, lanes, order)[0], g, f"map {i} by itself, variant {v}")


def test_records_only_each_plane_alone_and_a_short_struct():
    s, suns, want = R.case("random_bernoulli20", (33, 47), ALL16, 0)
    m = H.HostMap(s)
    R.assert_same_horizons(H.run_many([m], ALL16, 0, suns, planes=())[0], (want[0], None, want[2]), "records only")
    for p in R.PLANES:
        got = H.run_many([m], ALL16, 0, suns, planes=(p,))[0]
        assert list(got[1]) == [p]
        R.assert_same_horizons(got, want, f"{p} alone")
    short = H.run_many([m], ALL16, 0, suns, planes=(), struct_size=24)[0][0]
    for a, b in zip(short, want[0]):
        assert [a[f] for f in R.FIELDS[:6]] == [b[f] for f in R.FIELDS[:6]] and a["step_sum"] == 0xEEEEEEEEEEEEEEEE


# ---------------------------------------------------------------- 5. the sanitizers
def _dump(path, s, mask, reach, suns, want):
    recs, planes, counts = want
    out = (capi.Horizon * len(recs))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x5A524F48, s)
        f.write(struct.pack("<IIII", mask, reach, len(suns), 0))
        for d, t in suns:
            f.write(struct.pack("<IId", d, 0, t))
        for p, dt in (("slope", "<f8"), ("step", "<u4"), ("sky", "<f8"), ("open", "<u4"), ("lit", "<u4")):
            f.write(np.ascontiguousarray(planes[p], dt).tobytes())
        f.write(np.ascontiguousarray(counts, "<u4").tobytes())
        f.write(bytes(out))


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/horizons_host/horizons_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in,
    over its own inputs and over the restatement's results for the NaN and infinity map, the integer ties, a map with empty columns
    and lakes, and the one-cell-wide maps."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 11, out
    dumps = []
    for name, dims, mask, reach in (("nan_inf", (33, 47), ALL16, 0), ("integer_ties", (64, 64), ALL16, 5), ("empty", (96, 80), 0x0F0F, 0), ("ties", (1, 70), ALL16, 1),
                                    ("spike", (70, 1), 0x0101, 0)):
        s, suns, want = R.case(name, dims, mask, reach)
        dumps.append(str(tmp_path / f"{name}_{dims[0]}x{dims[1]}.bin"))
        _dump(dumps[-1], s, mask, reach, suns, want)
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out


# ---------------------------------------------------------------- 6. the binding's helpers and the refusals that need no device
def test_the_helpers_of_the_binding():
    assert capi.horizon_mask(0x8001) == 0x8001 and capi.horizon_mask([0, 15]) == 0x8001 and capi.horizon_mask([(1, 0), (2, -1)]) == 0x8001
    assert capi.horizon_mask(range(16)) == 0xFFFF and capi.horizon_mask(np.arange(4)) == 0xF
    with pytest.raises(ValueError):
        capi.horizon_mask([(3, 1)])
    with pytest.raises(ValueError):
        capi.horizon_mask([16])
    for d, (ux, uy) in enumerate(R.DIRS):
        az = math.degrees(math.atan2(uy, ux))
        assert capi.horizon_direction(az, 45.0)[0] == capi.horizon_direction(az + 360.0, 45.0)[0] == capi.horizon_direction(az + 5.0, 0.0)[0] == d
    assert capi.horizon_direction(0.0, 45.0)[1] == math.tan(math.radians(45.0)) and capi.horizon_direction(-1.0, 0.0) == (0, 0.0)
    assert capi.horizon_direction(13.0, 0.0)[0] == 0 and capi.horizon_direction(14.0, 0.0)[0] == 1          # halfway to atan2(1, 2) = 26.57 degrees
    with pytest.raises(ValueError):
        capi.horizon_direction(0.0, 90.0)
    suns = capi.horizon_suns([(90.0, 30.0), (4, 0.5), capi.Sun(7, 0, 2.0)])
    assert [(x.direction, x.reserved, x.tangent) for x in suns] == [(4, 0, math.tan(math.radians(30.0))), (4, 0, 0.5), (7, 0, 2.0)]


def test_refused_arguments_without_a_device():
    lib = capi.load()
    assert {"smx_horizons", "smx_ensemble_horizons"} <= set(capi.SYMBOLS)
    HSZ = C.sizeof(capi.Horizon)
    out = (capi.Horizon * 17)()
    C.memset(out, 0xCA, C.sizeof(out))
    canary = bytes(out)
    counts = np.full(65, 0xCACACACA, np.uint32)
    planes = [np.full(16 * 64, -7.5), np.full(16 * 64, 0xCACACACA, np.uint32), np.full(64, -7.5), np.full(64, 0xCACACACA, np.uint32), np.full(64, 0xCACACACA, np.uint32)]
    pl = [capi.ptr(p) for p in planes]
    none = [None] * 5
    assert lib.smx_horizons(None, 0xFFFF, 0, out, HSZ, None, 0, None, *none) == -2
    assert lib.smx_ensemble_horizons(None, 0xFFFF, 0, out, HSZ, None, 0, None) == -2
    good = capi.horizon_suns([(0, 0.5), (3, 0.0)])
    far = capi.horizon_suns([(0, 0.5), (5, 0.0)])              # direction 5 is not in the mask 0x0F
    sixteen = capi.horizon_suns([(0, 0.5), (16, 0.0)])
    bad = {k: capi.horizon_suns([(0, 0.5), (3, v)]) for k, v in (("negative", -0.5), ("nan", float("nan")), ("inf", float("inf")))}
    h = C.c_void_p()
    rc = lib.smx_create(C.byref(capi.Config(8, 8, 80, 0, 4096, capi.ENGINE_SERIAL, 0)), C.byref(h))
    assert h, "a handle is handed out even without a device"
    c = capi.ptr(counts)
    refused = [
        ((0x0F, 0, out, 0, good, 2, c, *pl), b"struct_size is 0"),
        ((0x0F, 0, None, HSZ, good, 2, c, *pl), b"out is null"),
        ((0, 0, out, HSZ, None, 0, None, *pl[:4], None), b"directions is 0"),
        ((0x1000F, 0, out, HSZ, good, 2, c, *pl), b"a bit above 15"),
        ((0x0F, 0, out, HSZ, good, 65, c, *pl), b"nsuns is 65"),
        ((0x0F, 0, out, HSZ, None, 2, c, *pl), b"suns is null while nsuns is 2"),
        ((0x0F, 0, out, HSZ, good, 2, None, *pl), b"lit_cells is null while nsuns is 2"),
        ((0x0F, 0, out, HSZ, far, 2, c, *pl), b"suns[1].direction is 5, not a direction of the mask 15"),
        ((0x0F, 0, out, HSZ, sixteen, 2, c, *pl), b"suns[1].direction is 16"),
        ((0x0F, 0, out, HSZ, bad["negative"], 2, c, *pl), b"suns[1].tangent is -0.5"),
        ((0x0F, 0, out, HSZ, bad["nan"], 2, c, *pl), b"suns[1].tangent is"),
        ((0x0F, 0, out, HSZ, bad["inf"], 2, c, *pl), b"suns[1].tangent is inf"),
        ((0x0F, 0, out, HSZ, None, 0, None, *pl), b"lit is asked for while nsuns is 0"),
    ]
    try:
        for args, text in refused:
            assert lib.smx_horizons(h, *args) == -2 and b"smx_horizons: " in lib.smx_last_error(h) and text in lib.smx_last_error(h), (text, lib.smx_last_error(h))
            assert bytes(out) == canary and (counts == 0xCACACACA).all() and all((p == (-7.5 if p.dtype == np.float64 else 0xCACACACA)).all() for p in planes), text
        if rc != 0:                                            # no device: what is well-formed is refused for that, with -3
            assert lib.smx_horizons(h, 0x0F, 0, out, HSZ, good, 2, c, *pl) == -3 and b"without a device" in lib.smx_last_error(h)
            assert bytes(out) == canary and (counts == 0xCACACACA).all()
    finally:
        lib.smx_destroy(h)
    e = C.c_void_p()
    erc = lib.smx_ensemble_create(0, C.byref(e))
    try:
        if erc != 0:                                           # the handle of the failed create refuses the call with a text
            assert lib.smx_ensemble_horizons(e, 0x0F, 0, out, HSZ, good, 2, c) == -3 and b"smx_ensemble_horizons" in lib.smx_ensemble_last_error(e)
        else:                                                  # an empty ensemble: 0, nothing looked at and nothing written
            assert lib.smx_ensemble_horizons(e, 0, 0, None, HSZ, None, 0, None) == 0
        assert bytes(out) == canary and (counts == 0xCACACACA).all()
    finally:
        lib.smx_ensemble_destroy(e)
