"""Drainage on the CPU: soil_drain.h compiled by g++ (tests/drainage_host) against the independent restatement tests/drainage_ref.py.

Every record field, the count and the three planes must equal the restatement exactly (floats by their bits), for every tile shape,
every workgroup width and every launch order the host build offers -- the workgroups and the lanes, first to last and last to first:
nothing in the result may depend on them."""
import ctypes as C
import struct

import numpy as np
import pytest

from analysis_host_lib import drainage as H, build_check, run_check, write_columns
import drainage_ref as R
import lakes_ref
from common import golden_snapshot
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)


def _check_all_shapes(s, want, what, cap=None):
    """Every tile shape x width (and the other three launch orders on two of them) against `want`."""
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in ((0, 1, 2, 3) if v in (0, 2) else (0,)):
                recs, planes, n = H.run_many([m], v, lanes, order, cap)[0]
                tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}"
                k = len(want[0]) if cap is None else min(cap, len(want[0]))
                assert n == len(want[0]), f"{tag}: {n} basins counted, expected {len(want[0])}"
                R.assert_same_drainage((recs, planes), (want[0][:k], want[1]), tag)
                if cap is None:
                    R.assert_invariants(s, recs, planes, what=tag)


def test_variants_cover_three_tile_shapes_and_the_kernels_own():
    v = H.variants()
    assert len(v) >= 3 and v[0] == (16, 64, 512)
    assert all(slots >= max(WIDTHS) for _, _, slots in v.values())


@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims):
    s, want = R.case(name, dims)
    R.assert_invariants(s, want[0], want[1], what=f"the restatement, {name} {dims}")
    _check_all_shapes(s, want, f"{name} {dims}")


def test_the_inputs_are_what_they_are_meant_to_be():
    for dims in ((64, 64), (96, 80), (33, 47)):
        n = dims[0] * dims[1]
        recs, planes, extra = R.case("cone", dims)[1]
        assert len(recs) == 1 and recs[0]["cells"] == n and int(planes["area"].max()) == n, "cone: one sink, every path converges"
        for name in ("ramp_x", "ramp_y"):
            recs, planes, extra = R.case(name, dims)[1]
            assert len(recs) == 1 and int(extra["steps"].max()) >= max(dims) - 1, f"{name}: paths as long as the map is wide"
        recs, planes, extra = R.case("spiral", dims)[1]
        assert int(extra["steps"].max()) >= n // 4, "spiral: one path through a large part of the map"
        recs, planes, extra = R.case("plateau", dims)[1]
        assert len(recs) == n and all(r["cells"] == 1 for r in recs) and (planes["area"] == 1).all() and (planes["receivers"] == R.NONE).all()
        recs, planes, extra = R.case("ties", dims)[1]
        assert extra["ties"] > n // 8, "ties: equal lowest neighbours"
        recs, planes, extra = R.case("random_bernoulli20", dims)[1]
        assert any(r["flags"] & R.F_LAKE for r in recs) and any(not r["flags"] & R.F_LAKE for r in recs), "lakes as terminals next to sinks"


def test_ties_minus_zero_and_nan():
    s, (recs, planes, _) = R.case("ties", (33, 47))
    recv, n = planes["receivers"].reshape(-1), 33 * 47
    wet, h = R.heights(s)
    z, nan = n // 3, n // 2 + 3
    assert lakes_ref.bits(h[z]) == lakes_ref.bits(0.0) and lakes_ref.bits(h[z + 1]) == lakes_ref.bits(-0.0) and np.isnan(h[nan])
    assert recv[z] == R.NONE and recv[z + 1] == R.NONE, "-0.0 and +0.0 tie: neither is lower, both are sinks"
    assert recv[nan] == R.NONE and not (recv == nan).any(), "a NaN is never lower and never has a lower neighbour"
    by_first = {r["first_cell"]: r for r in recs}
    assert by_first[nan]["cells"] == 1 and np.isnan(by_first[nan]["height_min"]) and np.isnan(by_first[nan]["height_max"])
    assert lakes_ref.bits(by_first[z + 1]["height_min"]) == lakes_ref.bits(-0.0)
    # of two equal lowest neighbours the smaller index wins
    dimy = 47
    for c in range(n):
        if recv[c] != R.NONE:
            x, y = divmod(c, dimy)
            low = [u * dimy + v for u in range(max(0, x - 1), min(33, x + 2)) for v in range(max(0, y - 1), min(dimy, y + 2)) if h[u * dimy + v] == h[recv[c]]]
            assert recv[c] == min(low)


def test_corners_carry_the_border_bit():
    for dx, dy in ((64, 64), (96, 80), (33, 47)):
        s, (recs, planes, _) = R.case("corners", (dx, dy))
        lakes = [r for r in recs if r["flags"] & R.F_LAKE]
        assert [r["first_cell"] for r in lakes] == [0, dy - 1, (dx - 1) * dy, dx * dy - 1]
        assert all(r["flags"] == R.F_LAKE | R.F_BORDER and r["wet_cells"] == 1 for r in lakes)
        for r in recs:
            if not r["flags"] & R.F_LAKE:
                x, y = divmod(r["first_cell"], dy)
                assert bool(r["flags"] & R.F_BORDER) == (x in (0, dx - 1) or y in (0, dy - 1))
        assert any(r["flags"] == 0 for r in recs) and any(r["flags"] == R.F_BORDER for r in recs)


def test_cap_smaller_equal_and_larger_than_the_count():
    s, want = R.case("random_bernoulli20", (33, 47))
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5, 10 ** 4):
        _check_all_shapes(s, want, f"cap {cap}", cap=cap)


def test_maps_of_mixed_dimensions_in_one_launch():
    cases = [R.case("random_bernoulli20", (64, 64)), R.case("spiral", (33, 47)), R.case("plateau", (1, 70)), R.case("cone", (96, 80)), R.case("corners", (70, 1))]
    maps = [H.HostMap(s) for s, _ in cases]
    for v in VARIANTS:
        for lanes in WIDTHS:
            got = H.run_many(maps, v, lanes, v & 3)
            for (recs, planes, n), (_, want) in zip(got, cases):
                R.assert_same_drainage((recs, planes), want, f"mixed variant {v} lanes {lanes}", count=n)
            got = H.run_many(maps, v, lanes, 0, cap=3)          # a cap below one member's count: the counts stay, the records are cut
            for (recs, planes, n), (_, want) in zip(got, cases):
                assert n == len(want[0])
                R.assert_same_drainage((recs, planes), (want[0][:3], want[1]), f"mixed cap 3 variant {v} lanes {lanes}")
    # without the area plane the accumulation does not run, and nothing else changes
    got = H.run_many(maps, 0, 256, 0, planes=("receivers", "labels"))
    for (recs, planes, n), (_, want) in zip(got, cases):
        assert "area" not in planes
        R.assert_same_drainage((recs, planes), want, "no area plane", count=n)


# ---- the committed goldens: (lakes, wet cells, dry sinks, dry sinks on the border, ties, longest path, largest area at a dry cell) ----
GOLDENS = [("default64", 0, 0, 0, 99, 25, 0, 21, 202), ("default64", 20, 3, 399, 26, 26, 0, 54, 603), ("painted64", 5, 0, 0, 65, 23, 0, 59, 1188)]


@pytest.mark.parametrize("case,tick,lakes,wetcells,sinks,border,ties,longest,largest", GOLDENS, ids=[f"{c}.t{t}" for c, t, *_ in GOLDENS])
def test_goldens(case, tick, lakes, wetcells, sinks, border, ties, longest, largest):
    s = golden_snapshot(case, tick)
    want = R.drainage(s)
    recs, planes, extra = want
    wet, _ = R.heights(s)
    dry = [r for r in recs if not r["flags"] & R.F_LAKE]
    assert len(recs) - len(dry) == lakes and sum(r["wet_cells"] for r in recs) == wetcells == int(wet.sum())
    assert len(dry) == sinks and sum(1 for r in dry if r["flags"] & R.F_BORDER) == border
    assert extra["ties"] == ties and int(extra["steps"].max()) == longest
    assert int(planes["area"].reshape(-1)[~wet].max()) == largest
    if (case, tick) == ("default64", 20):
        assert sum(r["cells"] for r in recs if r["flags"] & R.F_LAKE) == 1843
    R.assert_invariants(s, recs, planes, what=f"{case}.t{tick}")
    _check_all_shapes(s, want, f"{case}.t{tick}")


def _dump(path, s, want):
    """An input and the restatement's result in the layout tests/drainage_host/drainage_check.cpp reads."""
    recs, planes, _ = want
    out = (capi.Basin * max(1, len(recs)))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x4E415244, s)
        f.write(struct.pack("<I", len(recs)))
        for p in R.PLANES:
            f.write(np.ascontiguousarray(planes[p], "<u4").tobytes())
        f.write(bytes(out)[:len(recs) * C.sizeof(capi.Basin)])


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/drainage_host/drainage_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in,
    over its own inputs and over every input of drainage_ref at every size, 128 x 128 included."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 11, out
    dumps = []
    for name, dims in R.all_cases():
        s, want = R.case(name, dims)
        dumps.append(str(tmp_path / f"{name}_{dims[0]}x{dims[1]}.bin"))
        _dump(dumps[-1], s, want)
    assert len(dumps) == 54 and {"spiral", "ties", "ramp_y", "random_checker", "corners", "empty"} <= {n for n, _ in R.all_cases()}
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
