"""The stream network on the CPU: soil_streams.h compiled by g++ (tests/streams_host) against the independent restatement
tests/streams_ref.py.

Every record field, the count and the four planes must equal the restatement exactly (doubles by their bits), for every tile shape,
every workgroup width and every launch order the host build offers -- the workgroups and the lanes, first to last and last to first:
nothing in the result may depend on them."""
import ctypes as C
import struct

import numpy as np
import pytest

import drainage_ref as D
from analysis_host_lib import streams as H, build_check, run_check, write_columns
import streams_ref as R
from common import golden_snapshot
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
NONE = R.NONE


def _check_all_shapes(s, threshold, want, what, cap=None, drain=None):
    """Every tile shape x width (and the other three launch orders on two of them) against `want`."""
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in ((0, 1, 2, 3) if v in (0, 2) else (0,)):
                recs, planes, n = H.run_many([m], threshold, v, lanes, order, cap)[0]
                tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}"
                k = len(want[0]) if cap is None else min(cap, len(want[0]))
                assert n == len(want[0]), f"{tag}: {n} segments counted, expected {len(want[0])}"
                R.assert_same_streams((recs, planes), (want[0][:k], want[1]), tag)
                if cap is None:
                    R.assert_invariants(s, threshold, recs, planes, drain=drain, what=tag)


def test_variants_are_the_drainage_host_builds():
    from analysis_host_lib import drainage as drainage_host_lib
    assert {v: t[:2] for v, t in drainage_host_lib.variants().items()} == H.variants() and H.variants()[0] == (16, 64)


@pytest.mark.parametrize("threshold", R.THRESHOLDS)
@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims, threshold):
    s, drain, want = R.case(name, dims, threshold)
    R.assert_invariants(s, threshold, want[0], want[1], drain=drain, what=f"the restatement, {name} {dims} threshold {threshold}")
    _check_all_shapes(s, threshold, want, f"{name} {dims} threshold {threshold}", drain=drain)


def test_the_inputs_are_what_they_are_meant_to_be():
    for dims in D.SIZES:
        # a plateau has no cell with an area above 1: no channel at all from threshold 2 on, every cell a one-cell segment at 1
        for t in (3, 8):
            recs, planes, extra = R.case("plateau", dims, t)[2]
            assert recs == [] and not extra["channel"].any() and (planes["segments"] == NONE).all() and not planes["order"].any()
        recs, planes, extra = R.case("plateau", dims, 1)[2]
        assert len(recs) == dims[0] * dims[1] and all(r["cells"] == 1 and r["flags"] & 6 == 6 for r in recs)
    for dims in ((33, 47), (1, 70), (70, 1)):                  # (at 64 x 64 and 96 x 80 one cell of `ties` gathers an area of 8)
        assert R.case("ties", dims, 8)[2][0] == []
    assert [len(R.case("ties", dims, 8)[2][0]) for dims in ((64, 64), (96, 80))] == [1, 1]
    # the long walk: the spiral trench is ONE segment of 2040 cells at 64 x 64 with threshold 8
    recs, planes, extra = R.case("spiral", (64, 64), 8)[2]
    assert len(recs) == 1 and recs[0]["cells"] == 2040 and recs[0]["flags"] & R.F_HEAD and int(planes["reach"].max()) == 2040
    recs, planes, extra = R.case("cone", (64, 64), 1)[2]
    assert sum(1 for r in recs if r["flags"] & R.F_SINK) == 1 and max(r["order"] for r in recs) >= 2, "cone: one sink, confluences on the way"
    recs, planes, extra = R.case("random_bernoulli20", (96, 80), 1)[2]
    assert any(r["flags"] & R.F_WET for r in recs) and any(r["flags"] & R.F_SINK for r in recs) and int(extra["donors"].max()) >= 3


# ---- the hand-built input, asserted literally on the restatement ----
def _c(x, y):
    return x * 16 + y


def test_hand_built_network():
    s, drain, (recs, planes, extra) = R.hand_case(1)
    recv = drain[1]["receivers"]
    for (x, y), (_, r) in R.HAND.items():                      # the layout drains as it was drawn
        assert recv[x, y] == (NONE if r is None else _c(*R.HAND_LOW_WET) if r == "wet" else _c(*r)), (x, y)
    assert int(extra["channel"].sum()) == len(R.HAND) == 35 and len(recs) == 22
    order, heads, reach, seg = planes["order"], planes["heads"], planes["reach"], planes["segments"]
    by = {r["first_cell"]: r for r in recs}
    # the confluences: donors' orders -> order
    assert order[1, 0] == order[3, 0] == 1 and order[2, 1] == 2                                    # (1,1) -> 2
    assert order[2, 2] == 2 and order[1, 2] == 1 and order[2, 3] == 2                              # (2,1) -> 2
    assert order[3, 4] == 2 and order[5, 4] == 2 and order[4, 5] == 3                              # (2,2) -> 3
    assert order[9, 0] == order[10, 0] == order[11, 0] == 1 and order[10, 1] == 2                  # (1,1,1) -> 2
    assert order[10, 3] == 2 and order[11, 3] == 2 and order[9, 3] == 1 and order[10, 4] == 3      # (2,2,1) -> 3
    assert order[5, 5] == 1 and order[4, 6] == 3                                                   # (3,1) -> 3
    assert heads[2, 1] == 2 and heads[2, 3] == 3 and heads[4, 5] == 5 and heads[4, 8] == 6 and heads[10, 1] == 3 and heads[10, 4] == 6
    assert reach[2, 1] == 2 and reach[4, 5] == 6 and reach[4, 8] == 9 and reach[10, 4] == 5 and reach[14, 15] == 4 and reach[8, 8] == 1
    assert not order[0, 0] and not heads[4, 9] and not reach[4, 9] and seg[4, 9] == NONE and seg[0, 0] == NONE
    # a confluence directly below a confluence: a one-cell segment
    r = by[_c(4, 5)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["flags"], r["heads"], r["straight"], r["diagonal"], r["area_first"], r["area_last"]) == \
        (_c(4, 5), 1, 3, _c(4, 6), 0, 5, 1, 0, 14, 14)
    # a segment entering a lake
    r = by[_c(4, 6)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["flags"], r["heads"], r["straight"], r["diagonal"], r["area_first"], r["area_last"]) == \
        (_c(4, 8), 3, 3, NONE, R.F_WET, 6, 3, 0, 16, 18)
    assert r["basin"] == 0 and r["height_first"] == 12.0 and r["height_last"] == 10.0              # (the water around the trees is one lake: its first cell)
    # a head that is a sink
    r = by[_c(8, 8)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["basin"], r["flags"], r["heads"], r["straight"], r["diagonal"]) == \
        (_c(8, 8), 1, 1, NONE, _c(8, 8), R.F_SINK | R.F_HEAD, 1, 0, 0)
    # a confluence that is a sink
    r = by[_c(10, 4)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["basin"], r["flags"], r["heads"], r["straight"], r["diagonal"], r["area_last"]) == \
        (_c(10, 4), 1, 3, NONE, _c(10, 4), R.F_SINK, 6, 0, 0, 12)
    # a last_cell on the border
    r = by[_c(14, 12)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["basin"], r["flags"], r["straight"], r["diagonal"], r["area_last"]) == \
        (_c(14, 15), 4, 1, NONE, _c(14, 15), R.F_SINK | R.F_HEAD | R.F_BORDER, 3, 0, 4)
    # segments of several cells with straight and diagonal steps, joined downstream
    r = by[_c(6, 1)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["flags"], r["heads"], r["straight"], r["diagonal"]) == (_c(5, 4), 4, 2, _c(4, 5), 0, 2, 2, 2)
    r = by[_c(12, 2)]
    assert (r["last_cell"], r["cells"], r["order"], r["down"], r["flags"], r["straight"], r["diagonal"]) == (_c(11, 3), 2, 2, _c(10, 4), 0, 0, 2)
    assert by[_c(1, 0)]["flags"] == R.F_HEAD | R.F_BORDER and by[_c(1, 0)]["down"] == _c(2, 1) and by[_c(1, 2)]["flags"] == R.F_HEAD
    assert R.orders(recs) == {1: 14, 2: 5, 3: 3}
    for t in (1, 2, 3):
        s, drain, want = R.hand_case(t)
        R.assert_invariants(s, t, want[0], want[1], drain=drain, what=f"hand-built, threshold {t}")
        _check_all_shapes(s, t, want, f"hand-built, threshold {t}", drain=drain)
    assert len(R.hand_case(3)[2][0]) == 7


def test_cap_smaller_equal_and_larger_than_the_count():
    s, drain, want = R.case("random_bernoulli20", (33, 47), 3)
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5):
        _check_all_shapes(s, 3, want, f"cap {cap}", cap=cap)


def test_maps_of_mixed_dimensions_in_one_launch():
    for t in (1, 8):
        cases = [R.case("random_bernoulli20", (64, 64), t), R.case("spiral", (33, 47), t), R.case("plateau", (1, 70), t), R.case("cone", (96, 80), t),
                 R.case("corners", (70, 1), t)]
        maps = [H.HostMap(s) for s, _, _ in cases]
        for v in VARIANTS:
            for lanes in WIDTHS:
                got = H.run_many(maps, t, v, lanes, v & 3)
                for (recs, planes, n), (_, _, want) in zip(got, cases):
                    R.assert_same_streams((recs, planes), want, f"mixed threshold {t} variant {v} lanes {lanes}", count=n)
                got = H.run_many(maps, t, v, lanes, 0, cap=3)      # a cap below one member's count: the counts stay, the records are cut
                for (recs, planes, n), (_, _, want) in zip(got, cases):
                    assert n == len(want[0])
                    R.assert_same_streams((recs, planes), (want[0][:3], want[1]), f"mixed cap 3 threshold {t} variant {v} lanes {lanes}")


def test_one_plane_at_a_time_against_all_planes():
    s, drain, want = R.case("random_checker", (96, 80), 3)
    for order in (0, 3):
        for p in R.PLANES:
            recs, planes, n = H.run(s, 3, 0, 256, order, planes=(p,))
            assert list(planes) == [p]
            R.assert_same_streams((recs, planes), want, f"{p} alone, order {order}", count=n)
        recs, planes, n = H.run(s, 3, 0, 256, order, planes=())
        R.assert_same_streams((recs, None), want, "no plane", count=n)
        # records cut and no segments plane: the segments beyond the cap are not walked, the count and the other planes stay
        recs, planes, n = H.run(s, 3, 0, 256, order, cap=2, planes=("order", "reach", "heads"))
        R.assert_same_streams((recs, planes), (want[0][:2], want[1]), "cap 2 without the segments plane", count=None)
        assert n == len(want[0])


# ---- the committed goldens: (case, tick, threshold, segments, orders, largest reach or None) ----
GOLDENS = [("default64", 20, 4, 573, {1: 354, 2: 149, 3: 53, 4: 17}, None), ("default64", 20, 1, 1861, None, 55),
           ("default64", 0, 16, 131, {1: 103, 2: 28}, None), ("painted64", 5, 4, 563, {1: 340, 2: 146, 3: 61, 4: 16}, None)]


@pytest.mark.parametrize("case,tick,threshold,segments,orders,reach", GOLDENS, ids=[f"{c}.t{t}.a{a}" for c, t, a, *_ in GOLDENS])
def test_goldens(case, tick, threshold, segments, orders, reach):
    s = golden_snapshot(case, tick)
    drain = D.drainage(s)
    want = R.streams(s, threshold, drain)
    recs, planes, extra = want
    assert len(recs) == segments
    if orders is not None:
        assert R.orders(recs) == orders
    if reach is not None:
        assert max(r["order"] for r in recs) == 5 and int(planes["reach"].max()) == reach
    R.assert_invariants(s, threshold, recs, planes, drain=drain, what=f"{case}.t{tick}")
    _check_all_shapes(s, threshold, want, f"{case}.t{tick} threshold {threshold}", drain=drain)


def _dump(path, s, threshold, want):
    """An input and the restatement's result in the layout tests/streams_host/streams_check.cpp reads."""
    recs, planes, _ = want
    out = (capi.Stream * max(1, len(recs)))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x4D525453, s)
        f.write(struct.pack("<II", int(threshold), len(recs)))
        for p in R.PLANES:
            f.write(np.ascontiguousarray(planes[p], "<u4").tobytes())
        f.write(bytes(out)[:len(recs) * C.sizeof(capi.Stream)])


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/streams_host/streams_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in,
    over its own inputs and over every input of drainage_ref at every size, 128 x 128 included, with thresholds 1, 3 and 8, and the
    hand-built input."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 11, out
    dumps = []
    for name, dims in R.all_cases():
        for t in R.THRESHOLDS:
            s, _, want = R.case(name, dims, t)
            dumps.append(str(tmp_path / f"{name}_{dims[0]}x{dims[1]}_a{t}.bin"))
            _dump(dumps[-1], s, t, want)
    s, _, want = R.hand_case(1)
    dumps.append(str(tmp_path / "hand_16x16_a1.bin"))
    _dump(dumps[-1], s, 1, want)
    assert len(dumps) == 54 * 3 + 1
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
