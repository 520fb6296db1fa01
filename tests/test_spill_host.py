"""Spill analysis on the CPU: soil_spill.h compiled by g++ (tests/spill_host) against the independent restatement tests/spill_ref.py.

Every record field, the count and the filled plane must equal the restatement exactly (floats by their bits), for every tile shape,
every workgroup width and every launch order the host build offers, and for relax sweeps of 1 and 3 workgroups that stride over the
boundary list as the library's capped launch does: the order and the stride decide how many sweeps the fill levels take, never where
they end. The filled plane is held against a heap priority flood that knows nothing of basins."""
import ctypes as C
import struct

import numpy as np
import pytest

import lakes_ref as L
from analysis_host_lib import spill as H, build_check, run_check, write_columns
import spill_ref as R
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
    128^2 two shapes, both ends. Then relax sweeps of 1 and 3 workgroups on the kernels' own shape: both widths, both ends."""
    capped = [(0, lanes, order, blocks) for blocks in CAPPED for lanes in WIDTHS for order in (0, 3)]
    if tuple(dims) == tuple(R.BIG):
        return [(0, 256, 0, FULL), (0, 64, 3, FULL), (2, 64, 0, FULL), (2, 256, 3, FULL)] + capped
    return [(v, lanes, order, FULL) for v in VARIANTS for lanes in WIDTHS for order in ((0, 1, 2, 3) if v in (0, 2) else (0,))] + capped


def _check_all_shapes(s, want, what, dims, cap=None):
    m = H.HostMap(s)
    for v, lanes, order, blocks in _runs(dims):
        res, (sweeps, batches) = H.run_many([m], v, lanes, order, cap, relax_blocks=blocks)
        recs, filled, n = res[0]
        tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}" + (f" relax_blocks {blocks}" if blocks != FULL else "")
        k = len(want[0]) if cap is None else min(cap, len(want[0]))
        assert n == len(want[0]), f"{tag}: {n} basins counted, expected {len(want[0])}"
        R.assert_same_spill((recs, filled), (want[0][:k], want[1]), tag)
        assert sweeps == batches * G and sweeps <= _bound(want[2]["rounds"]), f"{tag}: {sweeps} sweeps in {batches} batches, {want[2]['rounds']} Jacobi rounds"


def test_variants_cover_three_tile_shapes_and_the_kernels_own():
    v = H.variants()
    assert len(v) >= 3 and v[0] == (16, 64, 1024, 512)
    assert all(ps >= tx * ty and slots >= max(WIDTHS) for tx, ty, ps, slots in v.values())
    assert G >= 2


def _flood(name, s, filled, what):
    """filled against the heap priority flood: equal bit for bit on the inputs without wet cells, never above it on the others."""
    pf = R.priority_flood(s)
    if name in R.DRY_INPUTS:
        assert np.array_equal(R.bits(filled), R.bits(pf)), f"{what}: filled differs from the priority flood at {int((R.bits(filled) != R.bits(pf)).sum())} cells"
    else:
        kf, kp = R.keys(filled), R.keys(pf)
        assert all(a <= b for a, b in zip(kf, kp)), f"{what}: filled lies above the priority flood"


@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims):
    s, base, want = R.case(name, dims)
    what = f"{name} {dims}"
    R.assert_invariants(name, want[0], base[0], f"the restatement, {what}")
    _flood(name, s, want[1], what)
    _check_all_shapes(s, want, what, dims)


def test_the_new_inputs_are_what_they_are_meant_to_be():
    for dims in ((64, 64), (96, 80), (33, 47), (128, 128)):
        dx, dy = dims
        n = dx * dy
        # nested: the inner bowl and the moat both fill above their pour heights; the pit in the rim pours off the map
        recs = R.case("nested", dims)[2][0]
        assert len(recs) == 3 and sum(1 for r in recs if r["flags"] & R.F_NESTED) == 2
        pit = [r for r in recs if r["flags"] & R.F_OFFMAP]
        assert len(pit) == 1 and pit[0]["first_cell"] == (dx // 2) * dy and pit[0]["pour_height"] == 8.0 and pit[0]["storage_q40"] == 0
        inner = max((r for r in recs if r["flags"] & R.F_NESTED), key=lambda r: r["cells_below"])
        assert all(7.0 <= r["pour_height"] < 8.0 and 9.0 <= r["fill_height"] < 10.0 for r in recs if r["flags"] & R.F_NESTED)
        assert inner["fill_storage_q40"] > inner["storage_q40"] > 0
        # rim: one basin pours off the map, through the notch; everything inside leaves at 2.5, the cell behind the notch
        recs, filled, _ = R.case("rim", dims)[2]
        off = [r for r in recs if r["flags"] & R.F_OFFMAP]
        x, y = R.rim_notch(dx, dy)
        assert len(off) == 1 and off[0]["first_cell"] == off[0]["pour_cell"] == x * dy + y and off[0]["pour_height"] == off[0]["fill_height"] == 2.0
        assert all(r["fill_height"] == 2.5 for r in recs if not r["flags"] & R.F_OFFMAP)
        assert (filled[2:-2, 2:-2] == 2.5).all()
        # level_lake: one lake, levelled at 1.5, with freeboard; it crosses a tile edge of the kernels' own shape
        s, base, (recs, filled, _) = R.case("level_lake", dims)
        lake = [(r, b) for r, b in zip(recs, base[0]) if r["flags"] & R.F_LAKE]
        x0, x1, y0, y1 = R.lake_box(dx, dy)
        assert len(lake) == 1 and lake[0][1]["wet_cells"] == (x1 - x0) * (y1 - y0) and x0 // 16 != (x1 - 1) // 16
        r = lake[0][0]
        assert r["pour_height"] >= 2.0 and r["cells_below"] >= lake[0][1]["wet_cells"]
        freeboard = r["pour_height"] - R.LAKE_LEVEL
        assert r["storage_q40"] >= lake[0][1]["wet_cells"] * int(freeboard * 2 ** 40) and (filled[x0:x1, y0:y1] == r["fill_height"]).all()
        # chain: at least 64 basins in series, the way out at the last cell
        s, base, (recs, filled, extra) = R.case("chain", dims)
        p, xs = R.chain_layout(dx, dy)
        pits = [r for r in recs if r["first_cell"] // dy >= xs and r["pour_height"] == 1.0]
        assert len(pits) >= 64 and all(r["fill_height"] == 1.0 for r in pits) and extra["rounds"] >= 64
        out = [r for r in recs if r["flags"] & R.F_OFFMAP and r["pour_height"] == 0.5]
        assert len(out) == 1 and out[0]["pour_cell"] == n - 1
        # unreliable: the deep pit's difference is >= 2^24, the ringed sink's levels are NaN
        s, base, (recs, filled, _) = R.case("unreliable", dims)
        pit, sink, ring = R.unreliable_cells(dx, dy)
        by = {r["first_cell"]: r for r in recs}
        assert by[pit]["flags"] & (R.F_STORAGE | R.F_FILL_STORAGE) == R.F_STORAGE | R.F_FILL_STORAGE and by[pit]["cells_below"] >= 1
        assert np.isnan(by[sink]["pour_height"]) and np.isnan(by[sink]["fill_height"]) and by[sink]["flags"] & R.F_STORAGE and by[sink]["cells_below"] == 1
        assert all(c in by and np.isnan(by[c]["pour_height"]) and by[c]["cells_below"] == 0 for c in ring)
        assert np.isnan(filled.reshape(-1)[sink]) and not any(r["flags"] & (R.F_STORAGE | R.F_FILL_STORAGE) for c, r in by.items() if c not in (pit, sink))


def test_chain_the_order_decides_the_sweeps_not_the_levels():
    for dims in ((33, 47), (64, 64), (96, 80)):
        s, base, want = R.case("chain", dims)
        (up, fu, _), (su, bu) = H.run(s, 0, 256, 0)
        (down, fd, _), (sd, bd) = H.run(s, 0, 256, 3)
        assert su > G and bu >= 2, f"{dims}: ascending, {su} sweeps in {bu} batches"
        assert sd < su and bd < bu, f"{dims}: descending {sd} sweeps, ascending {su}"
        assert su <= _bound(want[2]["rounds"]) and sd <= _bound(want[2]["rounds"])
        R.assert_same_spill((up, fu), want, f"chain {dims} ascending")
        R.assert_same_spill((down, fd), (up, fu), f"chain {dims} descending against ascending")


ROUNDS = [("random_bernoulli20", (96, 80), 45), ("random_bernoulli20", (128, 128), 77)]


def test_jacobi_rounds_of_the_restatement():
    for name, dims, rounds in ROUNDS:
        assert R.case(name, dims)[2][2]["rounds"] == rounds
    for case, tick, rounds in (("default64", 0, 11), ("default64", 20, 3)):
        assert R.spill(golden_snapshot(case, tick))[2]["rounds"] == rounds


def test_cap_smaller_equal_and_larger_than_the_count_and_a_short_struct():
    s, base, want = R.case("random_bernoulli20", (33, 47))
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5, 10 ** 4):
        _check_all_shapes(s, want, f"cap {cap}", (33, 47), cap=cap)
    # a caller compiled against a shorter struct gets that prefix of each record, at its own stride
    m = H.HostMap(s)
    short = np.full(4 * n + 4, 0xFFFFFFFF, np.uint32)
    nb = np.zeros(1, np.uint32)
    sw, ba = C.c_uint32(), C.c_uint32()
    hs = (C.c_void_p * 1)(m.h)
    assert H.lib().sh_spill(hs, 1, 0, 256, 0, H.RELAX_BLOCKS, n, capi.ptr(short), 16, capi.ptr(nb), None, C.byref(sw), C.byref(ba)) == 0
    assert int(nb[0]) == n and (short[4 * n:] == 0xFFFFFFFF).all()
    for k, r in enumerate(want[0]):
        assert [int(v) for v in short[4 * k:4 * k + 4]] == [r["first_cell"], r["pour_cell"], r["pour_to"], r["to_basin"]]


def test_maps_of_mixed_dimensions_in_one_launch():
    cases = [R.case("random_bernoulli20", (64, 64)), R.case("nested", (33, 47)), R.case("plateau", (1, 70)), R.case("level_lake", (96, 80)), R.case("corners", (70, 1)),
             R.case("chain", (33, 47))]
    maps = [H.HostMap(s) for s, _, _ in cases]
    most = max(w[2]["rounds"] for _, _, w in cases)
    for v in VARIANTS:
        for lanes in WIDTHS:
            got, (sweeps, batches) = H.run_many(maps, v, lanes, v & 3)
            for (recs, filled, n), (_, _, want) in zip(got, cases):
                R.assert_same_spill((recs, filled), want, f"mixed variant {v} lanes {lanes}", count=n)
            assert sweeps <= _bound(most)
            got, _ = H.run_many(maps, v, lanes, 0, cap=3)              # a cap below one member's count: the counts stay, the records are cut
            for (recs, filled, n), (_, _, want) in zip(got, cases):
                assert n == len(want[0])
                R.assert_same_spill((recs, filled), (want[0][:3], want[1]), f"mixed cap 3 variant {v} lanes {lanes}")
    got, _ = H.run_many(maps, 0, 256, 0, filled=False)                # without the plane nothing else changes
    for (recs, filled, n), (_, _, want) in zip(got, cases):
        assert filled is None
        R.assert_same_spill((recs, None), want, "no filled plane", count=n)


# ---- the committed goldens: (basins, nested ones, Jacobi rounds, wet cells) ----
GOLDENS = [("default64", 0, 99, 23, 11, 0), ("default64", 20, 29, 0, 3, 399), ("rgps64", 10, None, None, None, 0), ("painted64", 5, None, None, None, None),
           ("default64", 5, None, None, None, None), ("rgps64", 3, None, None, None, None)]


@pytest.mark.parametrize("case,tick,basins,nested,rounds,wetcells", GOLDENS, ids=[f"{c}.t{t}" for c, t, *_ in GOLDENS])
def test_goldens(case, tick, basins, nested, rounds, wetcells):
    s = golden_snapshot(case, tick)
    base = R.D.drainage(s)
    want = R.spill(s, base)
    recs, filled, extra = want
    wet, _ = R.D.heights(s)
    if basins is not None:
        assert len(recs) == basins and sum(1 for r in recs if r["flags"] & R.F_NESTED) == nested and extra["rounds"] == rounds
    if wetcells is not None:
        assert int(wet.sum()) == wetcells
    if (case, tick) == ("default64", 20):                   # every dry basin sits on the border, the three lakes hold the depressions
        assert sum(1 for r in recs if r["flags"] & R.F_LAKE) == 3 and all(b["flags"] & R.D.F_BORDER for r, b in zip(recs, base[0]) if not r["flags"] & R.F_LAKE)
    R.assert_invariants(f"{case}.t{tick}", recs, base[0], f"{case}.t{tick}")
    pf = R.priority_flood(s)
    if not wet.any():
        assert (case, tick) not in (("default64", 20),)
        assert np.array_equal(R.bits(filled), R.bits(pf)), f"{case}.t{tick}: filled differs from the priority flood"
    else:
        assert all(a <= b for a, b in zip(R.keys(filled), R.keys(pf))), f"{case}.t{tick}: filled lies above the priority flood"
    if (case, tick) in (("default64", 0), ("rgps64", 10)):
        assert not wet.any(), "the two goldens the filled surface is held to the priority flood on"
    _check_all_shapes(s, want, f"{case}.t{tick}", (int(s.dimx), int(s.dimy)))


def _dump(path, s, want):
    """An input and the restatement's result in the layout tests/spill_host/spill_check.cpp reads."""
    recs, filled, _ = want
    out = (capi.Spill * max(1, len(recs)))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x4C495053, s)
        f.write(struct.pack("<I", len(recs)))
        f.write(bytes(out)[:len(recs) * C.sizeof(capi.Spill)])
        f.write(np.ascontiguousarray(filled, "<f8").tobytes())


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/spill_host/spill_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in, over its
    own inputs and over every input of spill_ref at every size, 128 x 128 included. Host code only; nothing is loaded into Python."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 9, out
    dumps = []
    for name, dims in R.all_cases():
        s, _, want = R.case(name, dims)
        dumps.append(str(tmp_path / f"{name}_{dims[0]}x{dims[1]}.bin"))
        _dump(dumps[-1], s, want)
    assert len(dumps) == 15 * 6 and set(R.NEW_INPUTS) <= {n for n, _ in R.all_cases()}
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
