"""Dispersed flow on the CPU: soil_disp.h compiled by g++ (tests/dispersal_host) against the independent restatement
tests/dispersal_ref.py.

Every record field and the three planes must equal the restatement exactly, for every tile shape, every workgroup width and every
launch order the host build offers -- the workgroups and the lanes, first to last and last to first, the flow launches also against
the order of the other launches (which takes the ready list last to first) and with one workgroup (which takes it in many strides):
nothing in the result may depend on them."""

import numpy as np
import pytest

from analysis_host_lib import dispersal as H, build_check, run_check
import dispersal_ref as R
import drainage_ref as D
import lakes_ref as L
from common import golden_snapshot

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
ONE = R.ONE
ORDERS = (0, 1, 2, 3)                      # the launch orders of tests/hillslopes_host
FLOW_ORDERS = (4, 8, 12, 7, 11)            # ... and the flow's workgroups and lanes against the order of the launches around it


def _check_all_shapes(s, want, what, exponent, cap=None):
    """Every tile shape x width (and the other launch orders on two of them) against `want`."""
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in ((ORDERS + FLOW_ORDERS) if v in (0, 2) else (0,)):
                for blocks in ((H.FLOW_BLOCKS, 1) if order in (0, 12) else (H.FLOW_BLOCKS,)):
                    recs, planes, n, rounds = H.run_many([m], exponent, v, lanes, order, blocks, cap)[0]
                    tag = f"{what} exponent {exponent} variant {H.variants()[v]} lanes {lanes} order {order} flow workgroups {blocks}"
                    k = len(want[0]) if cap is None else min(cap, len(want[0]))
                    R.assert_same_dispersal((recs, planes), (want[0][:k], want[1]), tag)
                    assert n == len(want[0]), f"{tag}: {n} basins counted, expected {len(want[0])}"


def test_variants_are_the_drainage_host_builds():
    from analysis_host_lib import drainage as drainage_host_lib
    assert drainage_host_lib.variants() == H.variants() and H.variants()[0] == (16, 64, 512)


@pytest.mark.parametrize("name,dims", D.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims):
    for e in R.EXPONENTS:
        s, drain, want = R.case(name, dims, e)
        R.assert_invariants(s, *want, what=f"the restatement, {name} {dims} exponent {e}")
        _check_all_shapes(s, want, f"{name} {dims}", e)


# ---- the hand-built input of dispersal_ref, the numbers written out by hand ----
def _c(x, y):
    return x * 16 + y


# Exponent 0: every lower neighbour gets the same fraction, int(2^24 / k) for k of them.
#  The corner (0, 0) = 103 has k = 3: f = 5592405 each, the shares are 5592405 (A = ONE) and the remainder ONE - 3 * 5592405 = 1 goes
#  to its receiver (0, 1), the smallest of the three equally low cells. (0, 0) belongs to the basin of (0, 1): that basin keeps
#  ONE + 5592406 = 22369622 and leaks 2 * 5592405 = 11184810; (1, 0) and (1, 1) each hold ONE + 5592405 = 22369621.
#  The divide (2, 8) = 105 has k = 8: an eighth each, no remainder. The floor cells (1, 8) and (3, 8) see both pits, k = 2: they hold
#  1 + 1/8 and halve it. The pit (2, 7) = 90 collects 1 (itself) + 1/8 (the divide) + 2 * 9/8 ((1, 7), (3, 7)) + 3 ((1, 6), (2, 6),
#  (3, 6)) + 2 * 9/16 = 7.5 cells, the pit (2, 9) = 95 likewise 1 + 1/8 + 2 * 9/8 + 3 + 2 * 9/16 = 7.5. The divide and the two floor
#  cells are labelled with the deeper pit: what they hand to (2, 9), (1, 9), (3, 9) is leakage, 3/8 + 2 * 9/16 = 1.5 cells.
#  The lake (8, 3), (8, 4): twelve cells drain to it in D8. (7, 3) = 104 and (9, 4) = 106 have k = 8 and hand 3/8 each to floor sinks
#  of the row beyond them: 0.75 cells leak out, 11.25 arrive; the largest dry area is 1 + 1/8, first at (7, 2).
#  The lake without dry land stands above the floor: four wet cells, nothing arrives, no dry cell, no peak.
# (first_cell, cells, flags, peak_cell, inflow_q24, leak_in_q24, leak_out_q24, peak_q24, givers, split_cells)
HAND = {
    0: {
        1: (_c(0, 1), 2, 2, _c(0, 1), 22369622, 0, 11184810, 22369622, 1, 1),
        16: (_c(1, 0), 1, 2, _c(1, 0), 22369621, 5592405, 0, 22369621, 0, 0),
        17: (_c(1, 1), 1, 0, _c(1, 1), 22369621, 5592405, 0, 22369621, 0, 0),
        _c(2, 7): (_c(2, 7), 9, 0, _c(2, 7), 15 * ONE // 2, 0, 3 * ONE // 2, 15 * ONE // 2, 8, 3),
        _c(2, 9): (_c(2, 9), 6, 0, _c(2, 9), 15 * ONE // 2, 3 * ONE // 2, 0, 15 * ONE // 2, 5, 0),
        _c(8, 3): (_c(8, 3), 12, 1, _c(7, 2), 45 * ONE // 4, 0, 3 * ONE // 4, 9 * ONE // 8, 10, 4),
        _c(12, 12): (_c(12, 12), 4, 1, R.NONE, 4 * ONE, 0, 0, 0, 0, 0),
    },
    # Exponent 1, the corner: s = 3, 3 and 3 * 0.7071..., W = 8.1213...; f = int(3 / W * 2^24) = 6197471 twice and 4382273 for the
    # diagonal; they sum to ONE - 1, the 1 goes to (0, 1).
    1: {
        1: (_c(0, 1), 2, 2, _c(0, 1), ONE + 6197472, 0, 6197471 + 4382273, ONE + 6197472, 1, 1),
        16: (_c(1, 0), 1, 2, _c(1, 0), ONE + 6197471, 6197471, 0, ONE + 6197471, 0, 0),
        17: (_c(1, 1), 1, 0, _c(1, 1), ONE + 4382273, 4382273, 0, ONE + 4382273, 0, 0),
        _c(12, 12): (_c(12, 12), 4, 1, R.NONE, 4 * ONE, 0, 0, 0, 0, 0),
    },
}


def check_hand(recs, planes, exponent):
    """The hand-written numbers (shared with the device test)."""
    assert len(recs) == 228
    by_first = {r["first_cell"]: r for r in recs}
    for first, w in HAND[exponent].items():
        got = tuple(by_first[first][f] for f in R.FIELDS)
        assert got == w, f"exponent {exponent}, basin of cell {first}: {got} vs {w}"
    a, d, r = (planes[p].reshape(-1) for p in R.PLANES)
    assert (int(d[0]), int(r[0]), int(a[0])) == (0, 3, ONE), "the corner: a leaf that splits three ways"
    assert (int(d[_c(2, 8)]), int(r[_c(2, 8)]), int(r[_c(1, 8)]), int(d[_c(1, 8)])) == (0, 8, 2, 1), "the divide and the floor cell beside it"
    assert (int(d[_c(8, 3)]), int(r[_c(8, 3)]), int(d[_c(8, 4)])) == (7, 0, 7), "a wet cell counts its seven dry neighbours, all higher, and gives nothing"
    assert not d[_c(12, 12)] and not r[_c(12, 12)] and int(a[_c(12, 12)]) == ONE, "the lake above the floor"
    if exponent == 0:
        assert int(a[_c(1, 8)]) == 9 * ONE // 8 and int(a[_c(7, 2)]) == 9 * ONE // 8 and int(a[_c(8, 3)]) + int(a[_c(8, 4)]) == 45 * ONE // 4


@pytest.mark.parametrize("exponent", (0, 1))
def test_hand_built_map(exponent):
    s, drain, want = R.hand_case(exponent)
    R.assert_invariants(s, *want, what="the restatement, hand-built")
    check_hand(*want, exponent)
    _check_all_shapes(s, want, "hand-built", exponent)
    recs, planes, n, rounds = H.run(s, exponent)
    check_hand(recs, planes, exponent)


def test_ramp_on_one_row_and_one_column_is_d8():
    """A ramp on one row or one column: every cell but the lowest has exactly one lower neighbour, so the whole area goes to the
    receiver, whatever the exponent. (A local peak of a random row has two and splits.)"""
    for dims in ((1, 70), (70, 1)):
        s, drain = D.case("ramp_x", dims)
        for e in (0, 1, 4, 16):
            recs, planes, n, rounds = H.run(s, e)
            assert np.array_equal(planes["area"], drain[1]["area"].astype(np.uint64) * ONE), f"ramp_x {dims} exponent {e}"
            assert int(planes["receivers"].max()) == 1 and len(recs) == 1 and recs[0]["leak_out_q24"] == 0 and recs[0]["split_cells"] == 0 and recs[0]["givers"] == 69
            R.assert_invariants(s, recs, planes, what=f"ramp_x {dims}")
        s, drain = D.case("random_bernoulli20", dims)
        recs, planes, n, rounds = H.run(s, 1)
        R.assert_same_dispersal((recs, planes), R.dispersal(s, 1, drain), f"random {dims}", count=n)
        assert int(planes["receivers"].max()) == 2


def _steps(dx, dy, high, low):
    """Random cells at `high`, the others at `low`: every slope is high - low or 0."""
    h = np.where(np.random.default_rng(3).random((dx, dy)) < 0.4, high, low)
    return L.make_snapshot(np.zeros((dx, dy), bool), np.full((dx, dy), 2.0 ** -11), h, ())


@pytest.mark.parametrize("high,low", [(1e200, 0.0), (1.0 + 3e-200, 1.0), (3e-200, 2e-200)], ids=["overflow", "absorbed", "underflow"])
def test_weights_that_overflow_or_underflow_fall_back_to_d8(high, low):
    """Exponent 4: 1e200^4 is infinite, 1e-200^4 is 0 -- W is not a positive finite number, every fraction is 0 and the remainder,
    all of A, goes to the receiver: the D8 area times ONE. (`absorbed`: 1 + 3e-200 == 1 in f64, a plateau.)"""
    s = _steps(23, 19, high, low)
    drain = D.drainage(s)
    want = R.dispersal(s, 4, drain)
    recs, planes, n, rounds = H.run(s, 4)
    R.assert_same_dispersal((recs, planes), want, "steps", count=n)
    assert np.array_equal(planes["area"], drain[1]["area"].astype(np.uint64) * ONE)
    assert int(planes["receivers"].max()) >= 2 or high == 1.0 + 3e-200
    R.assert_invariants(s, recs, planes, what="steps")
    # with exponent 1 the same maps do split (where there is a slope at all)
    recs1, planes1, _, _ = H.run(s, 1)
    R.assert_same_dispersal((recs1, planes1), R.dispersal(s, 1, drain), "steps, exponent 1")
    assert high == 1.0 + 3e-200 or not np.array_equal(planes1["area"], planes["area"])


def test_exponent_16_is_accepted_and_17_refused():
    s, drain = D.case("cone", (9, 7))
    recs, planes, n, rounds = H.run(s, 16)
    R.assert_same_dispersal((recs, planes), R.dispersal(s, 16, drain), "cone (9, 7) exponent 16", count=n)
    m = H.HostMap(s)
    assert H.rc([m], 16) == 0 and H.rc([m], 17) == -2 and H.rc([m], 0xFFFFFFFF) == -2
    with pytest.raises(AssertionError):
        R.dispersal(s, 17, drain)


def test_the_chain_through_every_cell_and_the_rounds():
    """ramp_x: every cell waits for the one before it -- one lane walks the whole map in one launch; a second launch finds nothing."""
    s, drain, want = R.case("ramp_x", (33, 47), 1)
    for blocks in (1, H.FLOW_BLOCKS):
        recs, planes, n, rounds = H.run(s, 1, flow_blocks=blocks)
        R.assert_same_dispersal((recs, planes), want, "ramp_x")
        assert 1 <= rounds <= 33 * 47
    assert len(recs) == 1 and recs[0]["inflow_q24"] == 33 * 47 * ONE == recs[0]["peak_q24"] and recs[0]["peak_cell"] == 0
    s, drain, want = R.case("plateau", (33, 47), 1)
    assert H.run(s, 1)[3] == 0 and all(r["inflow_q24"] == ONE and r["givers"] == 0 for r in want[0])


def test_caps_smaller_equal_and_larger_than_the_counts():
    s, drain, want = R.case("random_bernoulli20", (33, 47), 1)
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5):
        _check_all_shapes(s, want, f"cap {cap}", 1, cap=cap) if cap in (1, n + 5) else None
        recs, planes, cnt, rounds = H.run(s, 1, cap=cap)
        R.assert_same_dispersal((recs, planes), (want[0][:cap], want[1]), f"cap {cap}")   # the planes cover every basin
        assert cnt == n


def test_maps_of_mixed_dimensions_in_one_launch():
    which = (("random_bernoulli20", (33, 47)), ("cone", (9, 7)), ("ties", (1, 70)), ("empty", (65, 63)))
    for e in (0, 4):
        cases = [R.case(nm, dm, e) for nm, dm in which]
        maps = [H.HostMap(c[0]) for c in cases]
        for v, lanes, order, blocks in ((0, 256, 0, H.FLOW_BLOCKS), (2, 64, 15, 1), (1, 256, 4, 3)):
            for got, c in zip(H.run_many(maps, e, v, lanes, order, blocks), cases):
                R.assert_same_dispersal(got[:2], c[2], f"mixed, variant {v} order {order}", count=got[2])
        for got, c in zip(H.run_many(maps, e, cap=3), cases):
            R.assert_same_dispersal(got[:2], (c[2][0][:3], c[2][1]), "mixed, cap 3")
            assert got[2] == len(c[2][0])


def test_many_tiny_members_in_one_launch():
    """Eight 1 x 20 ramps and a 5 x 5 cone: together they have more working member-launches than a batch has launches, and fewer
    cells than that. The call counts launches, not members: it ends, and reports no more rounds than the largest member has cells."""
    which = [("ramp_x", (1, 20))] * 8 + [("cone", (5, 5))]
    for e in (0, 1):
        cases = [(D.INPUTS[nm](*dm),) for nm, dm in which]
        cases = [(c[0], R.dispersal(c[0], e)) for c in cases]
        maps = [H.HostMap(c[0]) for c in cases]
        for v, lanes, order, blocks in ((0, 256, 0, H.FLOW_BLOCKS), (2, 64, 15, 1), (0, 64, 12, H.FLOW_BLOCKS)):
            assert H.rc(maps, e, v, lanes, order, blocks) == 0
            got = H.run_many(maps, e, v, lanes, order, blocks)
            for g, c in zip(got, cases):
                R.assert_same_dispersal(g[:2], c[1], f"tiny members, variant {v} order {order}", count=g[2])
            assert 10 <= got[0][3] <= 25, f"{got[0][3]} rounds for members of at most 25 cells"


@pytest.mark.parametrize("case,tick", [("default64", 0), ("default64", 20), ("default64s7", 40), ("rgps64", 10), ("rocksand48x80", 5)])
def test_goldens(case, tick):
    s = golden_snapshot(case, tick)
    drain = D.drainage(s)
    for e in R.EXPONENTS:
        want = R.dispersal(s, e, drain)
        R.assert_invariants(s, *want, what=f"{case}.t{tick}")
        for v, lanes, order in ((0, 256, 0), (2, 64, 15)):
            got = H.run(s, e, v, lanes, order)
            R.assert_same_dispersal(got[:2], want, f"{case}.t{tick} exponent {e}", count=got[2])


def _dump(path, s, want, exponent):
    """An input and the restatement's result in the layout tests/dispersal_host/dispersal_check.cpp reads."""
    n = int(s.dimx) * int(s.dimy)
    with open(path, "wb") as f:
        np.array([int(s.dimx), int(s.dimy), exponent, len(want[0])], np.uint32).tofile(f)
        np.ascontiguousarray(s.count, np.uint32).tofile(f)
        np.array([int(np.sum(s.count))], np.uint32).tofile(f)
        np.ascontiguousarray(s.type, np.uint32).tofile(f)
        np.ascontiguousarray(s.size, np.float64).tofile(f)
        np.ascontiguousarray(s.floor, np.float64).tofile(f)
        for p in R.PLANES:
            np.ascontiguousarray(want[1][p].reshape(n)).tofile(f)
        for r in want[0]:
            np.array([r["first_cell"], r["cells"], r["flags"], r["peak_cell"]], np.uint32).tofile(f)
            np.array([r["inflow_q24"], r["leak_in_q24"], r["leak_out_q24"], r["peak_q24"]], np.uint64).tofile(f)
            np.array([r["givers"], r["split_cells"], 0, 0], np.uint32).tofile(f)


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/dispersal_host/dispersal_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in,
    run as a child process -- nothing sanitized is loaded into this interpreter. Its own maps first (a one-cell map and the smallest
    shapes among them), then inputs of this suite with the restatement's results."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert "dispersal_check: OK" in out, out[-4000:]
    dumps = []
    for k, (name, dims, e) in enumerate((("hand", (16, 16), 1), ("ties", (9, 7), 4), ("random_bernoulli20", (33, 47), 0), ("empty", (1, 70), 1), ("cone", (33, 47), 4))):
        s, drain, want = R.case(name, dims, e)
        dumps.append(str(tmp_path / f"case{k}.bin"))
        _dump(dumps[-1], s, want, e)
    out = run_check(exe, dumps)
    assert f"dispersal_check: OK ({len(dumps)} files)" in out, out[-4000:]
