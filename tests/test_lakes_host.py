"""The lake census on the CPU: soil_lakes.h compiled by g++ (tests/lakes_host) against the independent restatement tests/lakes_ref.py.

Every record field and the whole label plane must equal the restatement exactly (floats by their bits), for every tile shape, every
workgroup width and both launch orders the host build offers: nothing in the census may depend on them."""
import math

import numpy as np
import pytest

from analysis_host_lib import lakes as H
import lakes_ref as R
from common import golden_snapshot
from observe_ref import figures_ref

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
_case = R.case


def _check_all_shapes(s, want, what, cap=None):
    """Every tile shape x width (and the descending launch order on two of them) against `want`."""
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for desc in ((False, True) if v in (0, 2) else (False,)):
                recs, labels, n = H.run_many([m], v, lanes, desc, cap)[0]
                tag = f"{what} variant {H.variants()[v]} lanes {lanes} descending {desc}"
                assert n == len(want[0]), f"{tag}: nlakes {n}, expected {len(want[0])}"
                k = n if cap is None else min(cap, n)
                R.assert_same_census((recs, labels), (want[0][:k], want[1]), tag)


def test_variants_cover_three_tile_shapes_and_the_kernels_own():
    v = H.variants()
    assert len(v) >= 3 and v[0] == (16, 64, 512)
    assert all(slots >= max(WIDTHS) for _, _, slots in v.values())


@pytest.mark.parametrize("dims", R.SIZES, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_shape(name, dims):
    s, want = _case(name, dims)
    _check_all_shapes(s, want, f"{name} {dims}")


def test_no_wet_cell_is_no_lake():
    s, (recs, labels) = _case("none", (64, 64))
    assert recs == [] and (labels == R.DRY).all()
    assert H.run(s)[2] == 0


@pytest.mark.parametrize("name", ["diagonal", "antidiagonal"])
def test_diagonals_join_through_corners_only(name):
    for dims in ((64, 64), (96, 80), (33, 47)):
        s, (r8, _) = _case(name, dims)
        r4, _ = R.census(s, 4)
        n = min(dims)
        assert len(r8) == 1 and r8[0]["cells"] == n, "one lake under eight neighbours"
        assert len(r4) == n, "the input tells the neighbourhoods apart: one lake per cell under four"
        assert H.run(s)[2] == 1


def test_checkerboard_is_one_lake_under_eight_neighbours():
    s, (r8, _) = _case("checker", (64, 64))
    assert len(r8) == 1 and r8[0]["cells"] == 2048
    assert len(R.census(s, 4)[0]) == 2048


def test_chains_and_comb_are_one_lake_rooted_at_cell_0():
    for name in ("spiral", "serpentine", "comb"):
        for dims in ((64, 64), (96, 80), (33, 47)):
            _, (recs, _) = _case(name, dims)
            assert len(recs) == 1 and recs[0]["first_cell"] == 0, (name, dims)


def test_half_planes_stay_two_lakes():
    for name in ("halves_row", "halves_diag"):
        for dims in ((64, 64), (96, 80), (33, 47)):
            s, (recs, _) = _case(name, dims)
            assert len(recs) == 2, (name, dims)
            assert H.run(s)[2] == 2
    # a ONE-cell-thick dry diagonal does not separate under eight neighbours (corner steps cross it); it does under four
    s, (recs, _) = _case("thin_diag", (64, 64))
    assert len(recs) == 1 and len(R.census(s, 4)[0]) == 2


def test_corner_cells_flags_and_boxes():
    for dx, dy in ((64, 64), (96, 80), (33, 47)):
        s, _ = _case("corners", (dx, dy))
        recs, labels, n = H.run(s)
        assert n == 4
        assert [(r["x0"], r["y0"], r["x1"], r["y1"]) for r in recs] == [(0, 0, 0, 0), (0, dy - 1, 0, dy - 1), (dx - 1, 0, dx - 1, 0), (dx - 1, dy - 1, dx - 1, dy - 1)]
        assert all(r["flags"] == R.F_BORDER and r["cells"] == 1 for r in recs)
        assert [r["first_cell"] for r in recs] == [0, dy - 1, (dx - 1) * dy, dx * dy - 1]
    # an inner lake does not carry the border bit
    w = np.zeros((33, 47), bool)
    w[5:9, 7:30] = True
    recs, _, _ = H.run(R.make_snapshot(w))
    assert len(recs) == 1 and recs[0]["flags"] == 0 and (recs[0]["x0"], recs[0]["y0"], recs[0]["x1"], recs[0]["y1"]) == (5, 7, 8, 29)


def test_values_levels_minus_zero_and_over_range():
    s = R.values_case()
    want = R.census(s)
    assert len(want[0]) == 3
    a, b, c = want[0]
    assert a["level_min"] < a["level_max"] and a["flags"] == 0
    assert b["flags"] == R.F_BORDER and c["flags"] == R.F_BORDER | R.F_VOLUME
    assert c["depth_max"] == 16777216.0
    _check_all_shapes(s, want, "values")
    # a lake that is nothing but -0.0: the extremes keep the sign (-0 < +0), the volume is 0 and reliable
    w = np.zeros((33, 47), bool); w[4:6, 4:9] = True
    z = np.full((33, 47), 0.0); z[4, 4:9] = -0.0
    base = np.zeros((33, 47)); base[4, 4:9] = -0.0     # (-0 + -0 = -0, the level of those cells; 0 + 0 = +0 elsewhere)
    s2 = R.make_snapshot(w, z, base)
    want2 = R.census(s2)
    r = want2[0][0]
    assert R.bits(r["level_min"]) == R.bits(-0.0) and R.bits(r["level_max"]) == R.bits(0.0) and R.bits(r["depth_max"]) == R.bits(0.0)
    assert r["volume_q40"] == 0 and r["flags"] == 0
    _check_all_shapes(s2, want2, "minus zero")


def test_volume_sum_that_wraps_is_flagged():
    # 2^24 - 2^-20 is in range: floor(size * 2^40) = 2^64 - 2^20; three of them pass 2^64
    w = np.zeros((64, 64), bool); w[10, 10:13] = True; w[40, 40] = True
    size = np.full((64, 64), 16777216.0 - 2.0 ** -20)
    s = R.make_snapshot(w, size)
    want = R.census(s)
    assert want[0][0]["flags"] == R.F_VOLUME and want[0][0]["volume_q40"] == (3 * (2 ** 64 - 2 ** 20)) % 2 ** 64
    assert want[0][1]["flags"] == 0 and want[0][1]["volume_q40"] == 2 ** 64 - 2 ** 20
    _check_all_shapes(s, want, "wrap")


def test_cap_smaller_equal_and_larger_than_the_count():
    s, want = _case("bernoulli41", (33, 47))
    n = len(want[0])
    assert n == 29
    for cap in (0, 1, n - 1, n, n + 5, 10 ** 4):
        _check_all_shapes(s, want, f"cap {cap}", cap=cap)


def test_maps_of_mixed_dimensions_in_one_launch():
    cases = [_case("bernoulli41", (64, 64)), _case("spiral", (33, 47)), _case("none", (1, 70)), _case("comb", (96, 80)), _case("corners", (70, 1))]
    maps = [H.HostMap(s) for s, _ in cases]
    for v in VARIANTS:
        for lanes in WIDTHS:
            got = H.run_many(maps, v, lanes, v == 1)
            for (recs, labels, n), (_, want) in zip(got, cases):
                assert n == len(want[0])
                R.assert_same_census((recs, labels), want, f"mixed variant {v} lanes {lanes}")
            # a cap below one member's count: every count stays right, the records are cut
            got = H.run_many(maps, v, lanes, False, cap=3)
            for (recs, labels, n), (_, want) in zip(got, cases):
                assert n == len(want[0])
                R.assert_same_census((recs, labels), (want[0][:3], want[1]), f"mixed cap 3 variant {v} lanes {lanes}")


# ---- the committed goldens: the figures below were measured with an independent labelling ----
GOLDENS = [("default64", 20, 399, 3, 386), ("default64", 5, 261, 3, 258), ("default64s7", 40, 36, 1, 36), ("rgps64", 10, None, 0, None)]


@pytest.mark.parametrize("case,tick,wet,lakes,largest", GOLDENS, ids=[f"{c}.t{t}" for c, t, *_ in GOLDENS])
def test_goldens(case, tick, wet, lakes, largest):
    s = golden_snapshot(case, tick)
    want = R.census(s)
    assert len(want[0]) == lakes
    if wet is not None:
        assert sum(r["cells"] for r in want[0]) == wet
        assert max(r["cells"] for r in want[0]) == largest
    if (case, tick) == ("default64", 20):
        assert len(R.census(s, 4)[0]) == 5
    _check_all_shapes(s, want, f"{case}.t{tick}")
    # consistency with the figures the project already has
    recs, _, _ = H.run(s)
    fig = figures_ref(s)
    assert sum(r["cells"] for r in recs) == fig["wet_cells"]
    wetmask, size, _ = R.tops(s)
    exact = math.fsum(float(v) for v in size[wetmask])
    total = math.fsum(r["volume"] for r in recs)
    assert abs(total - exact) < fig["wet_cells"] * 2.0 ** -40 + math.ulp(exact) or fig["wet_cells"] == 0 and total == 0.0
    assert all(r["volume"] == r["volume_q40"] * 2.0 ** -40 for r in recs)
