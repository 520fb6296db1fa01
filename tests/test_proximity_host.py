"""Proximity on the host: the bodies of soil_prox.h compiled by g++ (tests/prox_host) against the plain-loop restatement
(tests/proximity_ref.py) -- every site pattern at every size, the workgroup widths 64, 128 and 256 in ascending and descending launch
order, the envelopes in the library's band count and in others, LIST and WATER mode, several maps at once, and the stand-alone
sanitizer program. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import lakes_ref
import proximity_ref as ref
from analysis_host_lib import build_check
from proximity_host_lib import proximity as H, run_check

RUNS = [(lanes, order) for lanes in (64, 128, 256) for order in (0, 1)] + [(64, 3), (256, 2)]   # (order bit 1: the lanes last to first as well)
WATER = ("none", "all", "checker", "spiral", "comb", "corners", "bernoulli20", "bernoulli41")
_dry = {}


def dry(dims):
    """A map without water: LIST mode looks at no cell's content."""
    if dims not in _dry:
        _dry[dims] = lakes_ref.make_snapshot(np.zeros(dims, bool))
    return _dry[dims]


def test_hand_worked():
    """5 x 5, the list [0, 24]: the anti-diagonal and (2, 2) tie and go to site 0."""
    recs, pl, n = ref.proximity(5, 5, [0, 24], bins=3, bin_width=2)
    assert n == 2
    assert {k: recs[0][k] for k in ("site", "sites", "cells", "dist2_max", "farthest_cell", "dist2_sum")} == \
        {"site": 0, "sites": 1, "cells": 15, "dist2_max": 16, "farthest_cell": 4, "dist2_sum": 100}
    assert {k: recs[1][k] for k in ("site", "sites", "cells", "dist2_max", "farthest_cell", "dist2_sum")} == \
        {"site": 24, "sites": 1, "cells": 10, "dist2_max": 9, "farthest_cell": 9, "dist2_sum": 40}
    assert all(pl["group"][i, 4 - i] == 0 for i in range(5)) and pl["group"][2, 2] == 0 and pl["nearest"][4, 0] == 0
    assert (recs[0]["x0"], recs[0]["y0"], recs[0]["x1"], recs[0]["y1"]) == (0, 0, 4, 4) and (recs[1]["x0"], recs[1]["y0"]) == (1, 1)
    assert recs[0]["flags"] == 1 and recs[1]["flags"] == 1
    assert recs[0]["buffers"].tolist() == [4, 9, 2] and recs[1]["buffers"].tolist() == [4, 6, 0]      # (r = 0..4 by hand, two to a bin)
    s = dry((5, 5))
    for lanes, order in RUNS:
        ref.assert_same_proximity(H.run(s, [0, 24], bins=3, bin_width=2, lanes=lanes, order=order), (recs, pl, n), f"5x5 lanes {lanes} order {order}")
    ref.assert_invariants(5, 5, (recs, pl, n), [0, 24], H.run(dry((5, 5)), ref.transposed_sites(5, 5, [0, 24]))[1])


@pytest.mark.parametrize("dims", ref.SIZES, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("name", list(ref.PATTERNS))
def test_list_mode(name, dims):
    """Every pattern as a list: records, rows and planes equal the restatement's in every width and launch order."""
    cl, want = ref.case(name, dims, 5, 3)
    s = dry(dims)
    if cl is None:                                  # no site: LIST mode needs one; WATER mode on the dry map is the no-site case
        got = H.run(s)
        assert got[2] == 0 and not got[0] and all((p == ref.NONE).all() for p in got[1].values())
        ref.assert_invariants(dims[0], dims[1], got, [])
        return
    for k, (lanes, order) in enumerate(RUNS):           # the library's bands in every width and order, and beside them the plain scan or three bands
        for bands in (None, (1, 3)[k % 2]):
            got = H.run(s, cl, bins=5, bin_width=3, lanes=lanes, order=order, variant=k % 4, bands=bands)
            ref.assert_same_proximity(got, want, f"{name} {dims} lanes {lanes} order {order} bands {bands}")
    t = H.run(dry((dims[1], dims[0])), ref.transposed_sites(dims[0], dims[1], cl))[1]
    ref.assert_invariants(dims[0], dims[1], want, cl, t, f"{name} {dims}")


@pytest.mark.parametrize("dims", [(33, 47), (96, 80), (70, 1)], ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("name", ("mirror", "column_pair", "last_column", "checker", "bernoulli1", "bernoulli20"))
def test_band_counts(name, dims):
    """The envelopes built in bands of columns: whatever the count -- one, a count no width is a multiple of, a band per column,
    more bands than columns -- the result is the restatement's, ties across a band's edge included."""
    cl, want = ref.case(name, dims, 5, 3)
    assert H.lib().ph_bands() >= 1
    for k, bands in enumerate((1, 2, 3, 5, 8, 16, dims[0], 1000)):
        lanes, order = RUNS[k % len(RUNS)]
        ref.assert_same_proximity(H.run(dry(dims), cl, bins=5, bin_width=3, lanes=lanes, order=order, bands=bands), want, f"{name} {dims} bands {bands}")


@pytest.mark.parametrize("name", ("corner", "column_pair", "bernoulli20"))
def test_list_planes_and_bins(name):
    """Each plane alone, records only, one bin and 64 bins of width 1: what is not asked for is not written."""
    dims = (33, 47)
    cl, _ = ref.case(name, dims)
    s = dry(dims)
    for bins, width in ((0, 1), (1, 1), (64, 1)):
        want = ref.case(name, dims, bins, width)[1]
        for planes in ((), ("nearest",), ("group",), ("dist2",)):
            got = H.run(s, cl, bins=bins, bin_width=width, planes=planes)
            assert set(got[1]) == set(planes)
            ref.assert_same_proximity(got, want, f"{name} bins {bins} planes {planes}")


@pytest.mark.parametrize("dims", [(64, 64), (33, 47), (1, 70), (70, 1)], ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("name", WATER)
def test_water_mode(name, dims):
    """The wet cells grouped by their lakes: the lake masks of the census's tests."""
    s, want = ref.water_case(name, dims, 4, 2)
    for k, (lanes, order) in enumerate(RUNS[::2]):
        ref.assert_same_proximity(H.run(s, bins=4, bin_width=2, lanes=lanes, order=order, variant=k % 4, bands=(None, 1, 3, 5)[k]), want, f"{name} {dims} lanes {lanes} order {order}")
    wet = np.flatnonzero(lakes_ref.census(s)[1].reshape(-1) != lakes_ref.DRY)
    ref.assert_invariants(dims[0], dims[1], want, wet, None, f"{name} {dims}")


def test_water_cap_and_count():
    """A cap below the lake count: the count is whole, the first records and their rows are written, the planes are whole."""
    s, want = ref.water_case("bernoulli20", (33, 47), 4, 2)
    assert want[2] > 5
    got = H.run(s, bins=4, bin_width=2, cap=5)
    ref.assert_same_proximity(got, (want[0][:5], want[1], want[2]), "cap 5")
    got = H.run(s, cap=0, planes=())
    assert got[2] == want[2] and not got[0]


def test_many_maps():
    """Several unequal maps in one call, as the ensemble lays them out: each equals its own run."""
    cl = np.array([69, 3, 40, 0, 17], np.uint32)           # inside the smallest member (70 cells), not in cell order
    dims = [(33, 47), (70, 1), (64, 64), (1, 70)]
    maps = [H.HostMap(dry(d)) for d in dims]
    for lanes, order in ((64, 0), (256, 1)):
        for d, got in zip(dims, H.run_many(maps, cl, bins=3, bin_width=2, lanes=lanes, order=order)):
            ref.assert_same_proximity(got, ref.proximity(d[0], d[1], cl, bins=3, bin_width=2), f"list, member {d}")
    names = ["bernoulli20", "none", "spiral", "all"]
    maps = [H.HostMap(ref.water_case(nm, d)[0]) for nm, d in zip(names, dims)]
    for lanes, order in ((64, 1), (256, 0)):
        for nm, d, got in zip(names, dims, H.run_many(maps, None, bins=4, bin_width=2, lanes=lanes, order=order)):
            ref.assert_same_proximity(got, ref.water_case(nm, d, 4, 2)[1], f"water, member {nm} {d}")


def test_sanitizer_program(tmp_path):
    """tests/prox_host/prox_check.cpp with the address and undefined-behaviour sanitizers, as a child process: the 1-wide maps and
    the map without a site among its inputs."""
    out = run_check(build_check(tmp_path, H))
    assert "three maps" in out and out.count("ok") >= 9
