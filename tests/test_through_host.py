"""Through-drainage on the CPU: soil_through.h compiled by g++ (tests/through_host) against the independent restatement
tests/through_ref.py.

Every record field, the count and both planes must equal the restatement exactly (floats by their bits), for every tile shape, every
workgroup width and every launch order the host build offers, and for relax sweeps, hop sweeps and an exit of 1 and 3 workgroups that
stride over the boundary list as the library's capped launches do: the order and the stride decide how many sweeps the levels and the
hop counts take and which lane finishes a walk, never a result. The restatement's levels and hop counts are held against a heap Dijkstra over the
basins that shares nothing with its Jacobi rounds."""
import ctypes as C
import struct

import numpy as np
import pytest

import drainage_ref as D
import lakes_ref as L
import spill_ref as S
from analysis_host_lib import through as H, build_check, run_check, write_columns
import through_ref as R
from common import golden_snapshot
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
G = H.batch()


def _bound(rounds):
    return -(-rounds // G) * G


CAPPED = (1, 3)                            # relax_blocks below a lane per cell: the workgroups stride over the boundary list
FULL = H.RELAX_BLOCKS


def _runs(dims):
    """(variant, lanes, order, relax_blocks). At full width every shape x width, all four launch orders on two of the shapes; at
    128^2 two shapes, both ends. Then sweeps and an exit of 1 and 3 workgroups on the kernels' own shape: both widths, both ends."""
    capped = [(0, lanes, order, blocks) for blocks in CAPPED for lanes in WIDTHS for order in (0, 3)]
    if tuple(dims) == tuple(R.BIG):
        return [(0, 256, 0, FULL), (0, 64, 3, FULL), (2, 64, 0, FULL), (2, 256, 3, FULL)] + capped
    return [(v, lanes, order, FULL) for v in VARIANTS for lanes in WIDTHS for order in ((0, 1, 2, 3) if v in (0, 2) else (0,))] + capped


def _check_all_shapes(s, want, what, dims, cap=None):
    m = H.HostMap(s)
    for v, lanes, order, blocks in _runs(dims):
        res, (lsw, hsw, batches) = H.run_many([m], v, lanes, order, cap, relax_blocks=blocks)
        recs, planes, n = res[0]
        tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}" + (f" relax_blocks {blocks}" if blocks != FULL else "")
        k = len(want[0]) if cap is None else min(cap, len(want[0]))
        assert n == len(want[0]), f"{tag}: {n} basins counted, expected {len(want[0])}"
        R.assert_same_through((recs, planes), (want[0][:k], want[1]), tag)
        assert lsw + hsw == batches * G and lsw % G == 0 and hsw % G == 0, f"{tag}: {lsw} + {hsw} sweeps in {batches} batches"
        assert 0 < lsw <= _bound(want[2]["level_rounds"]), f"{tag}: {lsw} level sweeps, {want[2]['level_rounds']} Jacobi rounds"
        assert 0 < hsw <= _bound(want[2]["hop_rounds"]), f"{tag}: {hsw} hop sweeps, {want[2]['hop_rounds']} Jacobi rounds"


def _check_restatement(s, base, sp, want, what):
    R.assert_invariants(s, want[0], want[1], base, sp[0], f"the restatement, {what}")
    lev, hops = R.dijkstra(s, base)
    assert lev == [L.key(r["fill_height"]) for r in want[0]], f"{what}: the heap's levels are not the restatement's"
    assert hops == [r["hops"] for r in want[0]], f"{what}: the heap's hop counts are not the restatement's"
    assert want[2]["roots"] >= 1 and want[2]["hop_rounds"] <= 129


def test_variants_cover_four_tile_shapes_and_the_kernels_own():
    v = H.variants()
    assert len(v) == 4 and v[0] == (16, 64, 1024, 512) and len({(tx, ty) for tx, ty, _, _ in v.values()}) == 4
    assert all(ps >= tx * ty and slots >= max(WIDTHS) for tx, ty, ps, slots in v.values())
    assert G >= 2


@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims):
    s, base, sp, want = R.case(name, dims)
    what = f"{name} {dims}"
    _check_restatement(s, base, sp, want, what)
    _check_all_shapes(s, want, what, dims)


def test_following_the_pour_points_loops_and_following_the_exits_does_not():
    """What the exits are for: on these inputs most walks along spill()'s to_basin never reach the edge of the map."""
    for name, dims, loops, basins in (("rim", (64, 64), 406, 407), ("random_bernoulli20", (128, 128), 2439, 2673)):
        s, base, sp, want = R.case(name, dims)
        to = {r["first_cell"]: r["to_basin"] for r in sp[0]}
        bad = 0
        for f in to:
            seen, a = set(), f
            while a != R.NONE and a not in seen:
                seen.add(a)
                a = to[a]
            bad += a != R.NONE
        assert (bad, len(to)) == (loops, basins)
    recs = R.case("plateau", (33, 47))[2][0]
    assert not any(r["flags"] & S.F_OFFMAP for r in recs), "plateau: no walk along to_basin ever ends"


def test_the_new_inputs_are_what_they_are_meant_to_be():
    for dims in ((64, 64), (96, 80), (33, 47), (128, 128)):
        dx, dy = dims
        # twins: the two pits pour into each other; the first leaves over the saddle (not its pour point), the second through the first
        s, base, sp, (recs, planes, extra) = R.case("twins", dims)
        a, b, saddle = R.twins_cells(dx, dy)
        by, pour = {r["first_cell"]: r for r in recs}, {r["first_cell"]: r for r in sp[0]}
        assert len(recs) == 3 and pour[a]["to_basin"] == b and pour[b]["to_basin"] == a
        assert by[a]["exit_cell"] == saddle and by[a]["exit_height"] == 3.0 and by[a]["flags"] & R.F_NOT_POUR and by[a]["hops"] == 2
        assert by[b]["down"] == a and by[b]["hops"] == 3 and by[b]["exit_height"] == 1.0 and by[b]["fill_height"] == 3.0
        assert by[a]["through_cells"] == by[a]["cells"] + by[b]["cells"] and by[a]["upstream_basins"] == 1
        root = [r for r in recs if r["flags"] & R.F_OFFMAP]
        assert len(root) == 1 and root[0]["through_cells"] == dx * dy and root[0]["upstream_basins"] == 2
        assert int(planes["through_area"].reshape(-1)[by[a]["exit_to"]]) > by[a]["through_cells"] - 1
        # ring: one root; the pit opposite the gap has two equally short ways round, and the smaller (c, n) decides
        s, base, sp, (recs, planes, extra) = R.case("ring", dims)
        assert extra["roots"] == 1 and extra["max_hops"] > 30 and (planes["outlets"] == planes["outlets"][0, 0]).all()
        far = max(recs, key=lambda r: r["hops"])
        ways = [r for r in recs if r["hops"] == far["hops"] - 1 and L.key(r["fill_height"]) == L.key(far["fill_height"])]
        assert len(ways) == 2, "two neighbours at hops - 1: two equally short ways"
        # lake_entry: a pit whose exit leads to a wet cell; what it sends arrives in the lake's wet cells
        s, base, sp, (recs, planes, extra) = R.case("lake_entry", dims)
        wet, _ = D.heights(s)
        entry = [r for r in recs if r["flags"] & R.F_WET_ENTRY]
        assert len(entry) == 1 and wet[entry[0]["exit_to"]] and entry[0]["exit_height"] == 1.75 and entry[0]["cells"] == 9
        assert int(planes["through_area"].reshape(-1)[entry[0]["exit_to"]]) >= 1 + entry[0]["through_cells"]
    # an entry cell nobody drains into: the area walk must start from what was put there
    s, base, sp, (recs, planes, extra) = R.case("random_bernoulli20", (64, 64))
    has = set(int(v) for v in base[1]["receivers"].reshape(-1))
    wet, _ = D.heights(s)
    assert sum(1 for r in recs if r["exit_to"] != R.NONE and r["exit_to"] not in has and not wet[r["exit_to"]]) > 100


def test_ring_the_order_decides_the_sweeps_not_the_result():
    for dims in ((33, 47), (64, 64)):
        s, base, sp, want = R.case("ring", dims)
        (up, pu, _), su = H.run(s, 0, 256, 0)
        (down, pd, _), sd = H.run(s, 0, 256, 3)
        assert su != sd, f"{dims}: {su} and {sd}"
        R.assert_same_through((up, pu), want, f"ring {dims} ascending")
        R.assert_same_through((down, pd), (up, pu), f"ring {dims} descending against ascending")


ROUNDS = [("random_bernoulli20", (128, 128), 77, 87), ("ring", (128, 128), 124, 124)]


def test_jacobi_rounds_of_the_restatement():
    for name, dims, level, hop in ROUNDS:
        extra = R.case(name, dims)[3][2]
        assert (extra["level_rounds"], extra["hop_rounds"]) == (level, hop)
    assert max(R.case(n, d)[3][2]["hop_rounds"] for n, d in R.all_cases() if n in ("chain", "rim", "random_checker")) <= 129


def test_cap_smaller_equal_and_larger_than_the_count_and_a_short_struct():
    s, base, sp, want = R.case("random_bernoulli20", (33, 47))
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5, 10 ** 4):
        _check_all_shapes(s, want, f"cap {cap}", (33, 47), cap=cap)
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    m = H.HostMap(s)
    short = np.full(4 * n + 4, 0xFFFFFFFF, np.uint32)
    nb = np.zeros(1, np.uint32)
    sw = np.zeros(3, np.uint32)
    hs = (C.c_void_p * 1)(m.h)
    assert H.lib().th_through(hs, 1, 0, 256, 0, H.RELAX_BLOCKS, n, capi.ptr(short), 16, capi.ptr(nb), None, None, capi.ptr(sw)) == 0
    assert int(nb[0]) == n and (short[4 * n:] == 0xFFFFFFFF).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["exit_cell"], r["exit_to"], r["down"]]


def test_maps_of_mixed_dimensions_in_one_launch():
    cases = [R.case("random_bernoulli20", (64, 64)), R.case("twins", (33, 47)), R.case("plateau", (1, 70)), R.case("lake_entry", (96, 80)), R.case("corners", (70, 1)),
             R.case("ring", (33, 47))]
    maps = [H.HostMap(c[0]) for c in cases]
    level = max(c[3][2]["level_rounds"] for c in cases)
    hop = max(c[3][2]["hop_rounds"] for c in cases)
    for v in VARIANTS:
        for lanes in WIDTHS:
            got, (lsw, hsw, batches) = H.run_many(maps, v, lanes, v & 3)
            for (recs, planes, n), c in zip(got, cases):
                R.assert_same_through((recs, planes), c[3], f"mixed variant {v} lanes {lanes}", count=n)
            assert lsw <= _bound(level) and hsw <= _bound(hop) and lsw + hsw == batches * G
            got, _ = H.run_many(maps, v, lanes, 0, cap=3)            # a cap below one member's count: the counts stay, the records are cut
            for (recs, planes, n), c in zip(got, cases):
                assert n == len(c[3][0])
                R.assert_same_through((recs, planes), (c[3][0][:3], c[3][1]), f"mixed cap 3 variant {v} lanes {lanes}")
    got, _ = H.run_many(maps, 0, 256, 0, planes=False)              # without the planes nothing else changes
    for (recs, planes, n), c in zip(got, cases):
        assert planes is None
        R.assert_same_through((recs, None), c[3], "no planes", count=n)


# ---- the committed goldens: (basins, roots, largest hops, largest through_cells, largest area of drainage()) ----
GOLDENS = [("default64", 20, 29, 26, 2, 2446, 603), ("rgps64", 10, 78, 17, 12, 1530, 318), ("default64", 0, None, None, None, None, None),
           ("painted64", 5, None, None, None, None, None)]


@pytest.mark.parametrize("case,tick,basins,roots,hops,largest,area", GOLDENS, ids=[f"{c}.t{t}" for c, t, *_ in GOLDENS])
def test_goldens(case, tick, basins, roots, hops, largest, area):
    s = golden_snapshot(case, tick)
    base = D.drainage(s)
    sp = S.spill(s, base)
    want = R.through(s, base, sp)
    what = f"{case}.t{tick}"
    if basins is not None:
        assert (len(want[0]), want[2]["roots"], want[2]["max_hops"], max(r["through_cells"] for r in want[0])) == (basins, roots, hops, largest)
        assert int(base[1]["area"].max()) == area and int(want[1]["through_area"].max()) >= largest
    _check_restatement(s, base, sp, want, what)
    _check_all_shapes(s, want, what, (int(s.dimx), int(s.dimy)))


def _dump(path, s, want):
    """An input and the restatement's result in the layout tests/through_host/through_check.cpp reads."""
    recs, planes, _ = want
    out = (capi.Through * max(1, len(recs)))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x55524854, s)
        f.write(struct.pack("<I", len(recs)))
        f.write(bytes(out)[:len(recs) * C.sizeof(capi.Through)])
        f.write(np.ascontiguousarray(planes["through_area"], "<u4").tobytes())
        f.write(np.ascontiguousarray(planes["outlets"], "<u4").tobytes())


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/through_host/through_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in, over
    its own inputs and over every input of through_ref at every size, 128 x 128 included. Host code only; nothing is loaded into Python."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 9, out
    dumps = []
    for name, dims in R.all_cases():
        s, _, _, want = R.case(name, dims)
        dumps.append(str(tmp_path / f"{name}_{dims[0]}x{dims[1]}.bin"))
        _dump(dumps[-1], s, want)
    assert len(dumps) == 18 * 6 and set(R.NEW_INPUTS) <= {n for n, _ in R.all_cases()}
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
