"""The flow paths on the CPU: soil_paths.h compiled by g++ (tests/flowpaths_host) against the independent restatement
tests/flowpaths_ref.py.

Every record field, both counts, the seven planes and the profile must equal the restatement exactly (doubles by their bits), for
every tile shape, every workgroup width and every launch order the host build offers -- the workgroups and the lanes, first to last
and last to first, the up-walk also against the order of the other launches: nothing in the result may depend on them."""
import ctypes as C
import struct

import numpy as np
import pytest

import drainage_ref as D
from analysis_host_lib import flowpaths as H, build_check, run_check, write_columns
import flowpaths_ref as R
from common import golden_snapshot
from soilmachine_amd import capi

VARIANTS = sorted(H.variants())            # four tile shapes, the kernels' own among them
WIDTHS = (64, 256)
NONE = R.NONE
ORDERS = (0, 1, 2, 3)                      # the launch orders of tests/hillslopes_host
UP_ORDERS = (4, 8, 12, 7, 11)              # ... and the up-walk's workgroups and lanes against the order of the launches around it


def _check_all_shapes(s, want, what, cap=None, drain=None):
    """Every tile shape x width (and the other launch orders on two of them) against `want`."""
    m = H.HostMap(s)
    cells = m.dimx * m.dimy
    for v in VARIANTS:
        for lanes in WIDTHS:
            for order in ((ORDERS + UP_ORDERS) if v in (0, 2) else (0,)):
                recs, planes, prof, n, npr, rounds = H.run_many([m], v, lanes, order, cap, profile_cap=cells)[0]
                tag = f"{what} variant {H.variants()[v]} lanes {lanes} order {order}"
                k = len(want[0]) if cap is None else min(cap, len(want[0]))
                assert rounds == R.rounds(cells), f"{tag}: {rounds} rounds"
                assert len(prof) == npr
                R.assert_same_flowpaths((recs, planes, prof), (want[0][:k], want[1], want[2]), tag, nprofile=npr)
                assert n == len(want[0]), f"{tag}: {n} basins counted, expected {len(want[0])}"


def test_variants_are_the_drainage_host_builds():
    from analysis_host_lib import drainage as drainage_host_lib
    assert drainage_host_lib.variants() == H.variants() and H.variants()[0] == (16, 64, 512)


def test_rounds_of_a_map():
    """12 rounds at 64 x 64, 24 at 4096 x 4096, never more than 32; the sizes of the suite give both parities."""
    assert [R.rounds(c) for c in (1, 2, 3, 4, 5, 6, 4096, 4097, 4096 * 4096, (1 << 32) - 2)] == [0, 0, 1, 2, 2, 3, 12, 12, 24, 32]
    assert [R.rounds(a * b) % 2 for a, b in D.SIZES + [D.BIG]] == [0, 1, 1, 1, 1, 0]


@pytest.mark.parametrize("name,dims", R.all_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_input(name, dims):
    s, drain, want = R.case(name, dims)
    R.assert_invariants(s, *want, drain=drain, what=f"the restatement, {name} {dims}")
    _check_all_shapes(s, want, f"{name} {dims}", drain=drain)


# ---- the hand-built input of flowpaths_ref, the numbers written out by hand ----
_c = R.cell
# (first_cell, cells, source_cell, terminal_cell, steps_max, diagonal, profile_at, flags, straight_sum, diagonal_sum, drop_source, drop_max)
HAND = {
    32: (_c(2, 2), 7, _c(2, 6), _c(2, 2), 4, 0, 32, 0, 13, 2, 4.0, 4.0),         # the sink with the confluence: the trunk beats the tributary
    90: (_c(6, 2), 7, _c(4, 2), _c(6, 2), 2, 0, 94, 1, 4, 2, 19.5, 20.5),         # the lake entered twice by two steps: the smaller source
    158: (_c(10, 10), 2, _c(10, 10), _c(10, 10), 0, 0, 164, 1, 0, 0, 0.0, 0.0),   # the lake without dry land: its first_cell alone
    213: (_c(14, 4), 3, _c(12, 2), _c(14, 4), 2, 2, 219, 0, 0, 3, 20.0, 20.0),    # the diagonal-only path
}


def check_hand(recs, planes, profile, nbasins, nprofile):
    """The hand-written numbers (shared with the device test)."""
    assert nbasins == len(recs) == 241 and nprofile == len(profile) == 249
    for k, w in HAND.items():
        r = recs[k]
        got = tuple(r[f] for f in R.FIELDS)
        assert got[:10] == w[:10] and [R.bits(v) for v in got[10:]] == [R.bits(v) for v in w[10:]], f"basin {k}: {got} vs {w}"
    assert recs[213]["length"] == 2 * 2.0 ** 0.5 and recs[32]["length"] == 4.0
    single = [r for k, r in enumerate(recs) if k not in HAND]
    assert all(r["cells"] == 1 and r["steps_max"] == 0 and r["source_cell"] == r["terminal_cell"] == r["first_cell"] and r["flags"] == 0 and
               R.bits(r["drop_max"]) == 0 and R.bits(r["drop_source"]) == 0 for r in single)      # the NaN sinks: drop +0.0, no subtraction
    assert list(profile[32:37]) == [_c(2, 6), _c(2, 5), _c(2, 4), _c(2, 3), _c(2, 2)]
    assert list(profile[94:97]) == [_c(4, 2), _c(5, 2), _c(6, 2)] and profile[164] == _c(10, 10) and list(profile[219:222]) == [_c(12, 2), _c(13, 3), _c(14, 4)]
    stem, up, src, term = planes["stem"], planes["upstream"], planes["source"], planes["terminal"]
    # the stem of the lake's basin is ONE path: the other entry, its two cells and the middle of the lake are off it
    assert [int(stem[x, y]) for x, y in ((4, 2), (5, 2), (6, 2))] == [0, 1, 2]
    assert all(stem[x, y] == NONE for x, y in ((8, 5), (7, 5), (6, 4), (6, 3), (10, 11)))
    assert up[6, 4] == 2 and src[6, 4] == _c(8, 5) and up[6, 2] == 2 and src[6, 2] == _c(4, 2) and up[6, 3] == 0 and src[6, 3] == _c(6, 3)
    assert term[8, 5] == _c(6, 4) and term[4, 2] == _c(6, 2) and term[6, 3] == _c(6, 3) and planes["diagonal"][8, 5] == 1 and planes["straight"][8, 5] == 1
    # the confluence: three steps arrive by the trunk, two by the tributary
    assert up[2, 3] == 3 and src[2, 3] == _c(2, 6) and up[2, 2] == 4 and up[1, 4] == 1 and src[1, 4] == _c(0, 4) and stem[1, 4] == NONE and stem[2, 3] == 3
    assert (planes["straight"][0, 4], planes["diagonal"][0, 4], planes["drop"][0, 4]) == (2, 1, 3.5)
    assert stem[10, 10] == 0 and term[10, 11] == _c(10, 11) and stem[12, 12] == 0 and R.bits(planes["drop"][12, 12]) == 0
    assert int((stem != NONE).sum()) == 249


def test_hand_built_map():
    s, drain, want = R.hand_case()
    check_hand(want[0], want[1], want[2], len(want[0]), len(want[2]))
    R.assert_invariants(s, *want, drain=drain, what="hand-built")
    got = H.run(s)
    check_hand(*got[:5])
    _check_all_shapes(s, want, "hand-built", drain=drain)


def test_the_long_path():
    """The spiral trench at 64 x 64: one basin, one stem of 2047 cells, twelve rounds."""
    s, drain, want = R.case("spiral", (64, 64))
    assert len(want[0]) == 1 and want[0][0]["steps_max"] == 2046 and len(want[2]) == 2047 and want[0][0]["source_cell"] == 0 and R.rounds(4096) == 12
    trench = {c: k for k, c in enumerate(D.spiral_order(64, 64))}     # the stem follows the trench and cuts its corners diagonally
    at = [trench[int(c)] for c in want[2]]
    assert at == sorted(at) and at[0] == 0 and at[-1] == len(trench) - 1 and 0 < want[0][0]["diagonal"] == int(want[1]["diagonal"][0, 0]) < 2046
    for v, lanes, order in ((0, 256, 0), (0, 64, 3), (2, 256, 5), (3, 64, 10)):
        got = H.run(s, v, lanes, order)
        assert got[5] == 12
        R.assert_same_flowpaths(got, want, f"spiral variant {v} lanes {lanes} order {order}", count=got[3], nprofile=got[4])


def test_plateau_every_cell_its_own_basin():
    for dims in D.SIZES:
        s, drain, want = R.case("plateau", dims)
        n = dims[0] * dims[1]
        assert len(want[0]) == n == len(want[2]) and (want[2] == np.arange(n)).all() and not want[1]["stem"].any()
        assert all(r["steps_max"] == 0 and r["profile_at"] == k for k, r in enumerate(want[0]))
        got = H.run(s)
        R.assert_same_flowpaths(got, want, f"plateau {dims}", count=got[3], nprofile=got[4])


def test_ramp_on_one_row_and_one_column():
    for dims in ((1, 70), (70, 1)):
        s, drain, want = R.case("ramp_x", dims)
        assert len(want[0]) == 1 and want[0][0]["steps_max"] == 69 and list(want[2]) == list(range(69, -1, -1)) and want[0][0]["diagonal"] == 0
        _check_all_shapes(s, want, f"ramp_x {dims}")


def test_ties_the_nan_cell_and_the_zero_pair():
    s, drain, want = R.case("ties", (33, 47))
    n = 33 * 47
    term, drop = want[1]["terminal"].reshape(n), want[1]["drop"].reshape(n)
    nan, z = n // 2 + 3, n // 3
    assert term[nan] == nan and R.bits(drop[nan]) == 0 and term[z] == z and term[z + 1] == z + 1 and not np.isnan(drop).any()
    _check_all_shapes(s, want, "ties 33x47", drain=drain)


def test_caps_smaller_equal_and_larger_than_the_counts():
    s, drain, want = R.case("random_bernoulli20", (33, 47))
    n, npr = len(want[0]), len(want[2])
    assert n > 8 and npr > n
    for cap in (0, 1, n - 1, n, n + 5):
        _check_all_shapes(s, want, f"cap {cap}", cap=cap)          # (the planes and the profile cover every basin whatever cap is)
    m = H.HostMap(s)
    for pcap in (0, 1, npr - 1, npr, npr + 5):
        for cap in (1, n):
            recs, planes, prof, nb, got_npr, _ = H.run_many([m], 0, 256, 0, cap, profile_cap=pcap)[0]
            assert got_npr == npr and nb == n and len(prof) == min(pcap, npr)
            R.assert_same_flowpaths((recs, planes, prof), (want[0][:cap], want[1], want[2]), f"profile_cap {pcap} cap {cap}")


def test_maps_of_mixed_dimensions_in_one_launch():
    cases = [R.case("random_bernoulli20", (64, 64)), R.case("spiral", (33, 47)), R.case("plateau", (1, 70)), R.case("cone", (96, 80)), R.case("corners", (70, 1))]
    maps = [H.HostMap(c[0]) for c in cases]
    for v in VARIANTS:
        for lanes in WIDTHS:
            got = H.run_many(maps, v, lanes, (v & 3) | ((v ^ 1) << 2))
            for (recs, planes, _, n, npr, rounds), c in zip(got, cases):
                assert rounds == R.rounds(96 * 80)                         # one round count for the call: the largest map's
                R.assert_same_flowpaths((recs, planes), c[2], f"mixed variant {v} lanes {lanes}", count=n, nprofile=npr)   # (profile_at: within the member)
            got = H.run_many(maps, v, lanes, 0, cap=3)            # a cap below one member's count: the counts stay, the records are cut
            for (recs, planes, _, n, npr, _), c in zip(got, cases):
                assert n == len(c[2][0]) and npr == len(c[2][2])
                R.assert_same_flowpaths((recs, planes), (c[2][0][:3], c[2][1]), f"mixed cap 3 variant {v} lanes {lanes}")


def test_one_plane_at_a_time_against_all_planes():
    s, drain, want = R.case("random_checker", (96, 80))
    for order in (0, 3):
        for p in R.PLANES:
            recs, planes, prof, n, npr, _ = H.run(s, 0, 256, order, planes=(p,), profile_cap=None)
            assert list(planes) == [p] and prof is None
            R.assert_same_flowpaths((recs, planes), want, f"{p} alone, order {order}", count=n, nprofile=npr)
        got = H.run(s, 0, 256, order, planes=())
        R.assert_same_flowpaths(got, want, "the profile alone", count=got[3], nprofile=got[4])
        got = H.run(s, 0, 256, order, planes=(), profile_cap=None)
        R.assert_same_flowpaths(got, want, "records only", count=got[3], nprofile=got[4])


# ---- the committed goldens: (case, tick, basins, the profile's length, the largest steps_max), computed by the restatement ----
GOLDENS = [("default64", 20), ("rgps64", 10), ("default64s7", 40)]


@pytest.mark.parametrize("case,tick", GOLDENS, ids=[f"{c}.t{t}" for c, t in GOLDENS])
def test_goldens(case, tick):
    s = golden_snapshot(case, tick)
    drain = D.drainage(s)
    want = R.flowpaths(s, drain)
    R.assert_invariants(s, *want, drain=drain, what=f"{case}.t{tick}")
    _check_all_shapes(s, want, f"{case}.t{tick}", drain=drain)


def _dump(path, s, want):
    """An input and the restatement's result in the layout tests/flowpaths_host/flowpaths_check.cpp reads."""
    recs, planes, profile = want
    out = (capi.Flowpath * max(1, len(recs)))()
    for k, r in enumerate(recs):
        for f in R.FIELDS:
            setattr(out[k], f, r[f])
    with open(path, "wb") as f:
        write_columns(f, 0x48544150, s)
        f.write(struct.pack("<II", len(recs), len(profile)))
        for p in R.PLANES:
            f.write(np.ascontiguousarray(planes[p], "<f8" if p == "drop" else "<u4").tobytes())
        f.write(np.ascontiguousarray(profile, "<u4").tobytes())
        f.write(bytes(out)[:len(recs) * C.sizeof(capi.Flowpath)])


def test_the_bodies_under_the_sanitizers(tmp_path):
    """tests/flowpaths_host/flowpaths_check.cpp: a program of its own with the address and undefined-behaviour sanitizers linked in,
    over its own inputs (a spiral, a random map with lakes, a plateau) and over the restatement's results for the hand-built map, the
    long path and a random map."""
    exe = build_check(tmp_path, H)
    out = run_check(exe)
    assert out.count(" ok") == 9, out
    dumps = []
    for name, (s, _, want) in (("hand_16x16", R.hand_case()), ("spiral_64x64", R.case("spiral", (64, 64))), ("random_33x47", R.case("random_bernoulli20", (33, 47))),
                               ("empty_96x80", R.case("empty", (96, 80))), ("ties_1x70", R.case("ties", (1, 70)))):
        dumps.append(str(tmp_path / f"{name}.bin"))
        _dump(dumps[-1], s, want)
    out = run_check(exe, dumps)
    assert out.count(" ok") == len(dumps), out
