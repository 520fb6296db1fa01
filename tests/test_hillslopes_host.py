"""The hillslopes on the CPU: soil_hills.h compiled by g++ (tests/hillslopes_host) against the independent restatement
tests/hillslopes_ref.py.

Every record field, the count and the five planes must equal the restatement exactly (doubles by their bits), for every tile shape,
every workgroup width and every launch order the host build offers -- the workgroups and the lanes, first to last and last to first:
nothing in the result may depend on them."""
import ctypes as C
import struct

import numpy as np
import pytest

import drainage_ref as D
from analysis_host_lib import hillslopes as H, build_check, run_check, write_columns
import hillslopes_ref as R
import streams_ref as S
from common import golden_snapshot
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
NONE = R.NONE


def _check_all_shapes(s, threshold, want, what, cap=None, drain=None, strm=None):
    """Every tile shape x width (and the other three launch orders on two of them) against `want`."""
    m = H.HostMap(s)
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in ((0, 1, 2, 3) if v in (0, 2) else (0,)):
                recs, planes, n, rounds = H.run_many([m], threshold, v, lanes, order, cap)[0]
                tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}"
                k = len(want[0]) if cap is None else min(cap, len(want[0]))
                assert n == len(want[0]), f"{tag}: {n} segments counted, expected {len(want[0])}"
                assert rounds == R.rounds(threshold, m.dimx * m.dimy), f"{tag}: {rounds} rounds"
                R.assert_same_hillslopes((recs, planes), (want[0][:k], want[1]), tag)
                if cap is None:
                    R.assert_invariants(s, threshold, recs, planes, drain=drain, strm=strm, what=tag)


def test_variants_are_the_drainage_host_builds():
    from analysis_host_lib import drainage as drainage_host_lib
    assert drainage_host_lib.variants() == H.variants() and H.variants()[0] == (16, 64, 512)


def test_rounds_of_a_bound():
    assert [R.rounds(t, 4096) for t in (1, 2, 3, 4, 5, 8, 9, 10, 64, 65, 66, 4096, 4097, 1 << 31)] == [0, 0, 1, 2, 2, 3, 3, 4, 6, 6, 7, 12, 12, 12]
    assert R.rounds(8, 1) == 0 and R.rounds(8, 2) == 0 and R.rounds(8, 3) == 1


@pytest.mark.parametrize("threshold", R.THRESHOLDS)
@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims, threshold):
    """Thresholds 1, 3 and 8 queue 0, 1 and 3 rounds: the result ends in either of the two sets of planes."""
    s, drain, strm, want = R.case(name, dims, threshold)
    R.assert_invariants(s, threshold, want[0], want[1], drain=drain, strm=strm, what=f"the restatement, {name} {dims} threshold {threshold}")
    assert want[2]["longest"] <= R.bound(threshold, dims[0] * dims[1])
    _check_all_shapes(s, threshold, want, f"{name} {dims} threshold {threshold}", drain=drain, strm=strm)


# ---- the hand-built input of streams_ref, the records written out by hand ----
def _c(x, y):
    return x * 16 + y


Q = 1 << 40
# threshold 3: (first_cell, cells, steps_max, farthest_cell, straight_sum, diagonal_sum, hand_max, hand_sum_q40, bank_cells, head_cells)
HAND_3 = [
    (_c(2, 1), 3, 1, _c(1, 0), 0, 3, 1.5, 7 * Q // 2, 3, 2),        # (1,0) and (3,0) enter at the head, (1,2) further down at (2,3)
    (_c(4, 5), 1, 1, _c(5, 5), 0, 1, 5.0, 5 * Q, 1, 0),             # (5,5) enters the trunk at (4,6): not at the confluence itself
    (_c(6, 1), 2, 1, _c(5, 0), 0, 2, 1.0, 2 * Q, 2, 2),
    (_c(10, 1), 3, 1, _c(9, 0), 1, 2, 1.0, 3 * Q, 3, 3),            # (10,0) straight, (9,0) and (11,0) diagonal
    (_c(10, 4), 1, 1, _c(9, 3), 0, 1, 1.75, 7 * Q // 4, 1, 1),      # the confluence that is a sink takes (9,3)
    (_c(12, 2), 2, 1, _c(13, 1), 0, 2, 1.0, 2 * Q, 2, 2),
    (_c(14, 14), 2, 2, _c(14, 12), 3, 0, 2.0, 3 * Q, 1, 2),         # (14,12) two straight steps, (14,13) one
]


def test_hand_built_network():
    s, drain, strm, (recs, planes, extra) = R.hand_case(1)
    # threshold 1: every dry cell is a channel cell -- 22 segments, no hillslope at all
    assert len(recs) == 22 and all(r["cells"] == 0 and r["farthest_cell"] == NONE and r["hand_max"] == 0.0 and r["steps_max"] == 0 for r in recs)
    assert [r["first_cell"] for r in recs] == [g["first_cell"] for g in strm[0]] and extra == {"longest": 0, "unchannelled": 0}
    dry = planes["entry"] != NONE
    assert int(dry.sum()) == 35 and (planes["entry"][dry] == np.flatnonzero(dry.reshape(-1))).all() and not planes["hand"].any()
    assert planes["hillslope"][4, 9] == NONE and planes["entry"][4, 9] == NONE and planes["hillslope"][8, 8] == strm[1]["segments"][8, 8]
    s, drain, strm, (recs, planes, extra) = R.hand_case(3)
    got = [(r["first_cell"], r["cells"], r["steps_max"], r["farthest_cell"], r["straight_sum"], r["diagonal_sum"], r["hand_max"], r["hand_sum_q40"],
            r["bank_cells"], r["head_cells"]) for r in recs]
    assert got == HAND_3 and all(r["flags"] == 0 for r in recs)
    # the lone cell (8, 8) is a sink off the channels: its own entry, unchannelled; (14, 12) is two steps above its segment
    assert planes["entry"][8, 8] == _c(8, 8) and planes["hillslope"][8, 8] == NONE and planes["hand"][8, 8] == 0.0
    assert planes["entry"][14, 12] == _c(14, 14) and planes["straight"][14, 12] == 2 and planes["diagonal"][14, 12] == 0 and planes["hand"][14, 12] == 2.0
    assert planes["hillslope"][14, 12] == 6 and planes["hillslope"][5, 5] == 1 and planes["entry"][5, 5] == _c(4, 6) and planes["diagonal"][5, 5] == 1
    assert extra == {"longest": 2, "unchannelled": 0}
    for t in (1, 2, 3):
        s, drain, strm, want = R.hand_case(t)
        R.assert_invariants(s, t, want[0], want[1], drain=drain, strm=strm, what=f"hand-built, threshold {t}")
        _check_all_shapes(s, t, want, f"hand-built, threshold {t}", drain=drain, strm=strm)


def test_the_long_path():
    """The spiral trench at 64 x 64 drains 4096 cells through one path of 2046 steps: twelve rounds, and at 4097 no channel at all."""
    for t, nrec, unchannelled in ((4096, 1, 0), (4097, 0, 4095)):
        s, drain, strm, want = R.case("spiral", (64, 64), t)
        assert len(want[0]) == nrec and want[2] == {"longest": 2046, "unchannelled": unchannelled} and R.rounds(t, 4096) == 12
        if nrec:
            assert want[0][0]["cells"] == 4095 and want[0][0]["steps_max"] == 2046 and want[0][0]["head_cells"] == 4095
        assert int((want[1]["straight"] + want[1]["diagonal"]).max()) == 2046
        for v, lanes, order in ((0, 256, 0), (0, 64, 3), (2, 256, 1), (3, 64, 2)):
            recs, planes, n, rounds = H.run(s, t, v, lanes, order)
            assert rounds == 12
            R.assert_same_hillslopes((recs, planes), want, f"spiral threshold {t} variant {v} lanes {lanes} order {order}", count=n)
        R.assert_invariants(s, t, want[0], want[1], drain=drain, strm=strm, what=f"spiral threshold {t}")
    assert [R.case("spiral", (64, 64), t)[3][2]["longest"] for t in (8, 64)] == [7, 63]     # the bound is tight


def test_cone_paths_at_the_bound_and_below_it():
    for t, longest in ((64, 63), (1000, 64)):
        s, drain, strm, want = R.case("cone", (128, 128), t)
        assert want[2]["longest"] == longest == max(r["steps_max"] for r in want[0])
        for v, lanes, order in ((0, 256, 0), (2, 64, 3)):
            recs, planes, n, rounds = H.run(s, t, v, lanes, order)
            assert rounds == R.rounds(t, 128 * 128) == (6 if t == 64 else 10)
            R.assert_same_hillslopes((recs, planes), want, f"cone threshold {t} variant {v}", count=n)
        R.assert_invariants(s, t, want[0], want[1], drain=drain, strm=strm, what=f"cone threshold {t}")


def test_ties_the_nan_cell_and_the_zero_pair():
    s, drain, strm, want = R.case("ties", (33, 47), 3)
    n = 33 * 47
    entry, hand = want[1]["entry"].reshape(n), want[1]["hand"].reshape(n)
    nan, z = n // 2 + 3, n // 3
    # a NaN is never lower and never has a lower neighbour: a sink, its own entry, hand +0.0 -- no subtraction is made
    assert entry[nan] == nan and S.bits(hand[nan]) == 0 and want[1]["hillslope"].reshape(n)[nan] == NONE
    # -0 and +0 tie: neither drains into the other, both are their own entries unless a channel runs through them
    assert entry[z] == z and entry[z + 1] == z + 1 and S.bits(hand[z]) == 0 and S.bits(hand[z + 1]) == 0
    assert not np.isnan(hand).any()
    _check_all_shapes(s, 3, want, "ties 33x47 threshold 3", drain=drain, strm=strm)


def test_plateau_has_no_record():
    for dims in D.SIZES:
        for t in (3, 8):
            s, drain, strm, want = R.case("plateau", dims, t)
            assert want[0] == [] and want[2] == {"longest": 0, "unchannelled": 0} and (want[1]["hillslope"] == NONE).all()
            assert (want[1]["entry"].reshape(-1) == np.arange(dims[0] * dims[1])).all()
            recs, planes, n, _ = H.run(s, t)
            R.assert_same_hillslopes((recs, planes), want, f"plateau {dims} threshold {t}", count=n)


def test_cap_smaller_equal_and_larger_than_the_count():
    s, drain, strm, want = R.case("random_bernoulli20", (33, 47), 3)
    n = len(want[0])
    assert n > 8
    for cap in (0, 1, n - 1, n, n + 5):
        _check_all_shapes(s, 3, want, f"cap {cap}", cap=cap)


def test_maps_of_mixed_dimensions_in_one_launch():
    for t in (1, 8):
        cases = [R.case("random_bernoulli20", (64, 64), t), R.case("spiral", (33, 47), t), R.case("plateau", (1, 70), t), R.case("cone", (96, 80), t),
                 R.case("corners", (70, 1), t)]
        maps = [H.HostMap(c[0]) for c in cases]
        for v in VARIANTS:
            for lanes in WIDTHS:
                got = H.run_many(maps, t, v, lanes, v & 3)
                for (recs, planes, n, rounds), c in zip(got, cases):
                    assert rounds == R.rounds(t, 96 * 80)                  # one round count for the call: the largest map's
                    R.assert_same_hillslopes((recs, planes), c[3], f"mixed threshold {t} variant {v} lanes {lanes}", count=n)
                got = H.run_many(maps, t, v, lanes, 0, cap=3)    # a cap below one member's count: the counts stay, the records are cut
                for (recs, planes, n, _), c in zip(got, cases):
                    assert n == len(c[3][0])
                    R.assert_same_hillslopes((recs, planes), (c[3][0][:3], c[3][1]), f"mixed cap 3 threshold {t} variant {v} lanes {lanes}")


def test_one_plane_at_a_time_against_all_planes():
    s, drain, strm, want = R.case("random_checker", (96, 80), 8)
    for order in (0, 3):
        for p in R.PLANES:
            recs, planes, n, _ = H.run(s, 8, 0, 256, order, planes=(p,))
            assert list(planes) == [p]
            R.assert_same_hillslopes((recs, planes), want, f"{p} alone, order {order}", count=n)
        recs, planes, n, _ = H.run(s, 8, 0, 256, order, planes=())
        R.assert_same_hillslopes((recs, None), want, "no plane", count=n)


# ---- the committed goldens: (case, tick, threshold, segments, the sum of cells, the largest steps_max), computed by the restatement ----
GOLDENS = [("default64", 20, 4, 573, 2235, 3), ("default64", 20, 16, 114, 2915, 14), ("rgps64", 10, 4, 645, 2681, 3), ("rgps64", 10, 16, 118, 3494, 11),
           ("default64s7", 40, 4, 663, 2409, 3), ("default64s7", 40, 16, 110, 3387, 14)]


@pytest.mark.parametrize("case,tick,threshold,segments,cells,steps", GOLDENS, ids=[f"{c}.t{t}.a{a}" for c, t, a, *_ in GOLDENS])
def test_goldens(case, tick, threshold, segments, cells, steps):
    s = golden_snapshot(case, tick)
    drain = D.drainage(s)
    strm = S.streams(s, threshold, drain)
    want = R.hillslopes(s, threshold, drain, strm)
    recs = want[0]
    assert (len(recs), sum(r["cells"] for r in recs), max(r["steps_max"] for r in recs)) == (segments, cells, steps)
    R.assert_invariants(s, threshold, recs, want[1], drain=drain, strm=strm, what=f"{case}.t{tick}")
    _check_all_shapes(s, threshold, want, f"{case}.t{tick} threshold {threshold}", drain=drain, strm=strm)


def _dump(path, s, threshold, want):
    """An input and the restatement's result in the layout tests/hillslopes_host/hillslopes_check.cpp reads."""
    recs, planes, _ = want
    out = (capi.Hillslope * max(1, len(recs)))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x4C4C4948, s)
        f.write(struct.pack("<II", int(threshold), len(recs)))
        for p in R.PLANES:
            f.write(np.ascontiguousarray(planes[p], "<f8" if p == "hand" else "<u4").tobytes())
        f.write(bytes(out)[:len(recs) * C.sizeof(capi.Hillslope)])


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/hillslopes_host/hillslopes_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked
    in, over its own inputs and over every input of drainage_ref at every size, 128 x 128 included, with thresholds 1, 3 and 8, the
    hand-built input and the long path."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 11, out
    dumps = []
    for name, dims in R.all_cases():
        for t in R.THRESHOLDS:
            s, _, _, want = R.case(name, dims, t)
            dumps.append(str(tmp_path / f"{name}_{dims[0]}x{dims[1]}_a{t}.bin"))
            _dump(dumps[-1], s, t, want)
    s, _, _, want = R.hand_case(3)
    dumps.append(str(tmp_path / "hand_16x16_a3.bin"))
    _dump(dumps[-1], s, 3, want)
    s, _, _, want = R.case("spiral", (64, 64), 4096)
    dumps.append(str(tmp_path / "spiral_64x64_a4096.bin"))
    _dump(dumps[-1], s, 4096, want)
    assert len(dumps) == 54 * 3 + 2
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
