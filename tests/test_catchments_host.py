"""The catchments of listed outlets on the CPU: soil_catch.h compiled by g++ (tests/catchments_host) against the independent
restatement tests/catchments_ref.py.

Every record field, the four planes and the hypsometry tables must equal the restatement exactly (doubles by their bits), for every
tile shape, every workgroup width and every launch order the host build offers -- the workgroups and the lanes, first to last and last
to first: nothing in the result may depend on them. The host build runs the library's own round count, and the sizes of the suite give
both parities of it, so the fold reads either of the two sets."""
import ctypes as C
import struct

import numpy as np
import pytest

import catchments_ref as R
import drainage_ref as D
import flowpaths_ref as F
from catchments_host_lib import catchments as H, build_check, run_check, write_columns
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
NONE = R.NONE
ORDERS = (0, 1, 2, 3)
EDGE = 2.0 ** -7                            # the inputs' heights are multiples of 2^-10: a bin_height with many drops exactly on an edge
TINY = 2.0 ** -12                           # ... and one below every drop but +0.0: all cells but the entries land in the last bin


def _check_all_shapes(s, cells, want, what, bins=0, bin_height=1.0, orders=True):
    """Every tile shape x width (and the other launch orders on two of them) against `want`."""
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in (ORDERS if orders and v in (0, 2) else (0,)):
                recs, planes, hist, rounds = H.run_many([m], cells, v, lanes, order, bins=bins, bin_height=bin_height)[0]
                tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}"
                assert rounds == R.rounds(m.dimx * m.dimy), f"{tag}: {rounds} rounds"
                R.assert_same_catchments((recs, planes, hist), want, tag)


def test_variants_are_the_drainage_host_builds():
    from analysis_host_lib import drainage as drainage_host_lib
    assert drainage_host_lib.variants() == H.variants() and H.variants()[0] == (16, 64, 512)


def test_rounds_of_a_map():
    """12 rounds at 64 x 64, 13 at 96 x 80, 11 at 33 x 47: the sizes of the suite give both parities."""
    assert [R.rounds(a * b) for a, b in D.SIZES + [D.BIG]] == [12, 13, 11, 7, 7, 14]


@pytest.mark.parametrize("name,dims", D.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims):
    """One gauge at the lowest dry cell, every 7th cell, every cell and a seeded 5 % sample on every input."""
    paths = F.case(name, dims)[2]
    for which in ("lowest", "every7", "every", "sample"):
        bins = {"every7": 7, "sample": 64}.get(which, 0)
        s, drain, cells, want = R.case(name, dims, which, bins, EDGE)
        what = f"{name} {dims} {which}"
        R.assert_invariants(s, cells, *want, drain=drain, paths=paths, what=f"the restatement, {what}")
        if which == "every":
            area = drain[1]["area"].reshape(-1)
            assert all(r["cells"] == 1 and r["steps_max"] == 0 and r["straight_sum"] == r["diagonal_sum"] == 0 and r["area"] == int(area[r["cell"]])
                       for r in want[0] if drain[1]["receivers"].reshape(-1)[r["cell"]] != NONE)
            assert all(r["cells"] == 1 and r["farthest_cell"] == r["cell"] for r in want[0])
        _check_all_shapes(s, cells, want, what, bins, EDGE, orders=which in ("every7", "sample"))


@pytest.mark.parametrize("name", ["random_bernoulli20", "plateau"])
def test_wet_cells_and_sinks_only(name):
    for dims in ((64, 64), (33, 47)):
        s, drain, cells, want = R.case(name, dims, "terminals")
        wet, _ = D.heights(s)
        assert all(r["downstream"] == NONE and r["flags"] & 6 == (2 if wet[r["cell"]] else 4) for r in want[0])
        assert sum(r["cells"] for r in want[0]) == dims[0] * dims[1] and not (want[1]["gauge"] == NONE).any()      # every path ends at one of them
        paths = F.case(name, dims)[2]
        assert np.array_equal(want[1]["straight"], paths[1]["straight"]) and np.array_equal(want[1]["drop"].view(np.uint64), paths[1]["drop"].view(np.uint64))
        R.assert_invariants(s, cells, *want, drain=drain, paths=paths, what=f"{name} {dims} terminals")
        _check_all_shapes(s, cells, want, f"{name} {dims} terminals")


def check_line(s, drain, cells, want):
    """The spiral with every 100th cell of the way down from cell 0 (shared with the device test): a chain of nested gauges whose
    downstream pointers form one line. Between two gauges lie 100 steps of the trench, so the cell below the upper gauge is 99 steps
    from the lower one; a wall cell that drains into that cell from the side adds one."""
    recs, planes, _ = want
    n = len(cells)
    assert n >= 20 and [r["downstream"] for r in recs] == list(range(1, n)) + [NONE]
    recv = drain[1]["receivers"].reshape(-1)
    steps = (planes["straight"] + planes["diagonal"]).reshape(-1)
    for i in range(1, n):
        below = int(recv[cells[i - 1]])                     # the first trench cell of gauge i's own catchment
        assert int(planes["gauge"].reshape(-1)[below]) == i and int(steps[below]) == 99
        assert recs[i]["steps_max"] in (99, 100) and recs[i]["area"] == recs[i - 1]["area"] + recs[i]["cells"]
    assert recs[0]["steps_max"] == 100                       # cell 0 itself, the start of the walk, is not listed


def test_nested_gauges_along_the_spiral():
    for dims in ((64, 64), (96, 80), (128, 128)):
        s, drain, cells, want = R.case("spiral", dims, "path100", 7, EDGE)
        check_line(s, drain, cells, want)
        R.assert_invariants(s, cells, *want, drain=drain, paths=F.case("spiral", dims)[2], what=f"spiral {dims}")
        _check_all_shapes(s, cells, want, f"spiral {dims} path100", 7, EDGE)


# ---- the hand-built input of catchments_ref, every number written out by hand ----
# (cell, cells, area, downstream, basin, steps_max, farthest_cell, flags, straight_sum, diagonal_sum, drop_max, drop_sum_q40)
HAND = [
    (22, 2, 7, NONE, 15, 1, 17, 4, 1, 0, 2.0, 2 << 40),      # the sink (4, 2): itself and (3, 2); everything on the two arms lies above it
    (12, 3, 5, 0, 15, 2, 4, 0, 0, 3, 1.5, 2 << 40),          # the confluence (2, 2): itself and the shorter arm (1, 3), (0, 4), two diagonal steps
    (6, 2, 2, 1, 15, 1, 0, 0, 0, 1, 1.0, 1 << 40),           # (1, 1): itself and (0, 0)
]
_N = NONE
HAND_GAUGE = [[2, _N, _N, _N, 1], [_N, 2, _N, 1, _N], [_N, _N, 1, _N, _N], [_N, _N, 0, _N, _N], [_N, _N, 0, _N, _N]]
HAND_STRAIGHT = [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 0, 1], [0, 0, 0, 0, 0]]
HAND_DIAGONAL = [[1, 0, 0, 0, 2], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
HAND_DROP = [[1.0, 0, 0, 0, 1.5], [0, 0, 0, 0.5, 0], [0, 0, 0, 0, 0], [0, 0, 2.0, 0, 4.5], [0, 0, 0, 0, 0]]     # (3, 4) above the lake's level 1.5
HAND_HIST = [[1, 0, 1], [2, 1, 0], [1, 1, 0]]               # bin_height 1.0: the drops 1.0 and 2.0 lie exactly on an edge, 2.0 in the last bin


def check_hand(recs, planes, hist):
    """The hand-written numbers (shared with the device test)."""
    assert len(recs) == 3
    for r, w in zip(recs, HAND):
        got = tuple(r[f] for f in R.FIELDS)
        assert got[:10] == w[:10] and R.bits(got[10]) == R.bits(w[10]) and got[11] == w[11], f"{got} vs {w}"
    assert [r["drop_sum"] for r in recs] == [2.0, 2.0, 1.0]
    assert planes["gauge"].tolist() == HAND_GAUGE and planes["straight"].tolist() == HAND_STRAIGHT and planes["diagonal"].tolist() == HAND_DIAGONAL
    assert np.array_equal(planes["drop"].view(np.uint64), np.array(HAND_DROP, np.float64).view(np.uint64))       # (+0.0 everywhere else: no NaN leaks)
    assert np.asarray(hist).tolist() == HAND_HIST


def test_hand_built_map():
    s, drain, cells, want = R.hand_case()
    check_hand(*want)
    R.assert_invariants(s, cells, *want, drain=drain, paths=F.flowpaths(s, drain), what="hand-built")
    got = H.run(s, cells, bins=3, bin_height=1.0)
    check_hand(*got[:3])
    _check_all_shapes(s, cells, want, "hand-built", 3, 1.0)


HYPSO = [("random_bernoulli20", (64, 64), "every7"), ("cone", (33, 47), "sample"), ("spiral", (96, 80), "path100"), ("ties", (33, 47), "every7")]


@pytest.mark.parametrize("name,dims,which", HYPSO, ids=[f"{n}-{d[0]}x{d[1]}-{w}" for n, d, w in HYPSO])
def test_hypsometry(name, dims, which):
    """1, 7 and 64 bins with drops exactly on the edges, and a bin_height that puts most cells into the last bin."""
    for bins, bh in ((1, EDGE), (7, EDGE), (64, EDGE), (64, TINY), (7, 1e300)):
        s, drain, cells, want = R.case(name, dims, which, bins, bh)
        recs, planes, hist = want
        assert hist.shape == (len(cells), bins) and [int(v) for v in hist.sum(axis=1)] == [r["cells"] for r in recs]
        own = planes["gauge"] != NONE
        drops = planes["drop"][own]
        if bh == EDGE and name != "ties":
            assert int((np.mod(drops, bh) == 0).sum()) > int(own.sum()) // 16          # (cells exactly on an edge, the entries not counted alone)
        if bh == TINY:
            assert int(hist[:, 0].sum()) == int((drops == 0).sum()) and int(hist[:, -1].sum()) == int((drops >= 63 * TINY).sum())
            assert which == "every7" or name == "ties" or int(hist[:, -1].sum()) > int(own.sum()) // 2          # (most cells: the last bin)
        if bh == 1e300:
            assert int(hist[:, 0].sum()) == int(own.sum())
        _check_all_shapes(s, cells, want, f"{name} {dims} {which} bins {bins} bin_height {bh}", bins, bh, orders=bins == 7)


def test_maps_of_mixed_dimensions_in_one_launch():
    """One list for every map, as an index into each map's own plane; one round count for the call: the largest map's."""
    names = [("random_bernoulli20", (64, 64)), ("spiral", (33, 47)), ("plateau", (1, 70)), ("cone", (96, 80)), ("corners", (70, 1))]
    snaps = [D.case(n, d) for n, d in names]
    cells = [69, 0, 35, 7, 68, 13]
    wants = [R.catchments(s, cells, 7, EDGE, d) for s, d in snaps]
    maps = [H.HostMap(s) for s, _ in snaps]
    for v in VARIANTS:
        for lanes in WIDTHS:
            got = H.run_many(maps, cells, v, lanes, v & 3, bins=7, bin_height=EDGE)
            for (recs, planes, hist, rounds), want in zip(got, wants):
                assert rounds == R.rounds(96 * 80)
                R.assert_same_catchments((recs, planes, hist), want, f"mixed variant {v} lanes {lanes}")


def test_one_plane_at_a_time_against_all_planes():
    s, drain, cells, want = R.case("random_checker", (96, 80), "sample")
    for order in (0, 3):
        for p in R.PLANES:
            recs, planes, hist, _ = H.run(s, cells, 0, 256, order, planes=(p,))
            assert list(planes) == [p] and hist is None
            R.assert_same_catchments((recs, planes, hist), want, f"{p} alone, order {order}")
        got = H.run(s, cells, 0, 256, order, planes=())
        assert got[1] == {}
        R.assert_same_catchments(got, want, "records only")


def test_a_short_struct_size_gives_the_prefix():
    s, drain, cells, want = R.case("cone", (33, 47), "sample")
    m = H.HostMap(s)
    recs = H.run_many([m], cells, struct_size=32)[0][0]
    for r, w in zip(recs, want[0]):
        assert not R.same(r, w, R.FIELDS[:8]) and r["straight_sum"] == r["diagonal_sum"] == r["drop_sum_q40"] == 0xEEEEEEEEEEEEEEEE


def test_area_is_folded_in_any_list_order():
    """The same gauges listed upstream first, downstream first and shuffled: positions change, the figures of a cell do not."""
    s, drain, cells, _ = R.case("spiral", (64, 64), "path100")
    by_cell = None
    for order in (cells, cells[::-1], [int(c) for c in np.random.default_rng(3).permutation(cells)]):
        want = R.catchments(s, order, drain=drain)
        got = H.run(s, order)
        R.assert_same_catchments(got, want, "spiral relisted")
        fig = {r["cell"]: (r["cells"], r["area"], NONE if r["downstream"] == NONE else order[r["downstream"]]) for r in got[0]}
        assert by_cell is None or fig == by_cell
        by_cell = fig


# ---- the committed goldens ----
GOLDENS = [("default64", 20), ("rgps64", 10)]


@pytest.mark.parametrize("case,tick", GOLDENS, ids=[f"{c}.t{t}" for c, t in GOLDENS])
def test_goldens(case, tick):
    from common import golden_snapshot
    s = golden_snapshot(case, tick)
    drain = D.drainage(s)
    paths = F.flowpaths(s, drain)
    for which in ("every7", "sample"):
        cells = R.LISTS[which](s, drain)
        want = R.catchments(s, cells, 32, 0.25, drain)
        R.assert_invariants(s, cells, *want, drain=drain, paths=paths, what=f"{case}.t{tick} {which}")
        _check_all_shapes(s, cells, want, f"{case}.t{tick} {which}", 32, 0.25)


def _dump(path, s, cells, want, bins, bin_height):
    """An input and the restatement's result in the layout tests/catchments_host/catchments_check.cpp reads."""
    recs, planes, hist = want
    out = (capi.Catchment * len(recs))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x48544143, s)
        f.write(struct.pack("<IId", len(cells), bins, bin_height))
        f.write(np.ascontiguousarray(cells, "<u4").tobytes())
        for p in R.PLANES:
            f.write(np.ascontiguousarray(planes[p], "<f8" if p == "drop" else "<u4").tobytes())
        if bins:
            f.write(np.ascontiguousarray(hist, "<u4").tobytes())
        f.write(bytes(out))


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/catchments_host/catchments_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in,
    over its own inputs and lists and over the restatement's results for the hand-built map, the line of gauges on the spiral, wet
    cells and sinks only, every cell of a map with empty columns and a one-cell-wide map with a NaN and a -0.0."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 9, out
    dumps = []
    for name, (s, _, cells, want), bins, bh in (("hand_5x5", R.hand_case(), 3, 1.0), ("spiral_64x64", R.case("spiral", (64, 64), "path100", 7, EDGE), 7, EDGE),
                                                ("terminals_33x47", R.case("random_bernoulli20", (33, 47), "terminals"), 0, 1.0),
                                                ("empty_96x80", R.case("empty", (96, 80), "every", 0, EDGE), 0, EDGE),
                                                ("ties_1x70", R.case("ties", (1, 70), "sample", 64, EDGE), 64, EDGE)):
        dumps.append(str(tmp_path / f"{name}.bin"))
        _dump(dumps[-1], s, cells, want, bins, bh)
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
