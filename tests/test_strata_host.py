"""The strata readers on the CPU: soil_strata.h compiled by g++ (tests/strata_host) against the independent restatement
tests/strata_ref.py -- every integer exactly, every float by its bits, at workgroup widths 64 and 256 and several grid sizes:
nothing may depend on the launch shape. Also the transect rule, and the sanitizer run of the stand-alone strata_check."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import strata_host_lib as H
import strata_ref as R
from common import golden_snapshot
from observe_ref import figures_ref
from soilmachine_amd import capi
from soilmachine_amd.machine import Layermap

DIMS = [(1, 1), (5, 7), (64, 1), (1, 64), (96, 80), (65, 63)]
SHAPES = [(64, 1), (64, 3), (64, 1000), (256, 1), (256, 7)]       # (lanes, workgroups): one workgroup, a strided grid, more workgroups than cells need
_cache = {}


def case(dims, shift=0):
    """(snapshot, host map, totals at 64 types) of a synthetic map, made once"""
    key = (dims, shift)
    if key not in _cache:
        s = R.synthetic(dims, shift)
        _cache[key] = (s, H.HostMap(s), R.totals(s, 64))
    return _cache[key]


def cases(dims):
    return [case(dims, sh) for sh in (range(R.NPATTERNS) if dims == (1, 1) else (0,))]     # (1 x 1: every pattern in turn is the one column)


# ---------------------------------------------------------------- the synthetic columns
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_totals(dims):
    for s, m, want in cases(dims):
        for lanes, nb in SHAPES:
            R.assert_same_totals(H.totals(m, 64, lanes, nb), want, f"{dims} lanes {lanes} workgroups {nb}")
        for nt in (1, 2, 5, 7, 63):
            R.assert_same_totals(H.totals(m, nt), R.totals(s, nt), f"{dims} ntypes {nt}")
        R.assert_same_totals(R.totals_np(s, 64), want, f"{dims}: the vectorised fold")
        assert sum(r["sections"] for r in want[0]) + want[1] == s.nsec


def test_what_the_synthetic_columns_hold():
    s, m, (rec, other) = case((96, 80))
    n = s.ncells // R.NPATTERNS
    assert int(s.count.max()) == R.DEEP, "a chain longer than any staging"
    assert other == n and rec[63]["sections"] == n, "type 64 is only counted, type 63 is the last record"
    assert rec[3]["cells"] == 2 * n and rec[3]["sections"] == 4 * n, "a column is counted once however often the type recurs"   # (patterns 5 and 10)
    assert rec[0]["top_cells"] == 2 * n and rec[0]["sections"] == 3 * n, "buried Air is a section, not a wet cell"
    assert rec[0]["top_cells"] == figures_ref(s)["wet_cells"]
    assert rec[1]["flags"] == 0, "-0.0 is 0 and raises nothing"
    assert rec[2]["flags"] == R.F_VOLUME | R.F_HELD and rec[3]["flags"] == R.F_VOLUME | R.F_HELD, "NaN, +inf (and their products)"
    assert rec[4]["flags"] == R.F_VOLUME | R.F_HELD and rec[5]["flags"] == R.F_VOLUME, "-1.0 (held: -0.5), 2^24 with sat 0"
    assert rec[7]["flags"] == R.F_HELD, "a negative saturation"
    assert rec[6]["flags"] == R.F_VOLUME and rec[6]["volume_q40"] == (2 * n * (2 ** 64 - 2 ** 20)) % 2 ** 64, "the sum wrapped"
    assert rec[6]["held_q40"] == n * (2 ** 34 - 1) and rec[2]["held_q40"] > 0, "sat on buried sections is folded"


def test_other_counts_type_64_and_above():
    s, m, (rec, other) = case((96, 80))
    n = s.ncells // R.NPATTERNS
    assert other == int((s.type >= 64).sum()) == n
    assert rec[63]["sections"] == n


def test_wrap_through_a_doctored_start():
    s, m, want = case((5, 7))
    start = (capi.SoilTotal * 64)()
    start[1].volume_q40 = 2 ** 64 - 1            # one unit short of a wrap
    start[2].held_q40 = 2 ** 64 - 1
    start[4].volume_q40 = 2 ** 64 - 1 - want[0][4]["volume_q40"]       # ends exactly at 2^64 - 1: no wrap
    for lanes, nb in SHAPES:
        got, _ = H.totals(m, 64, lanes, nb, start=start)
        assert got[1]["flags"] == want[0][1]["flags"] | R.F_VOLUME and got[1]["volume_q40"] == want[0][1]["volume_q40"] - 1
        assert got[2]["flags"] & R.F_HELD and got[2]["held_q40"] == want[0][2]["held_q40"] - 1
        assert got[4]["volume_q40"] == 2 ** 64 - 1 and got[4]["flags"] == want[0][4]["flags"]


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_thickness(dims):
    for s, m, _ in cases(dims):
        for types in R.TYPE_LISTS:
            want = R.thickness(s, types)
            for lanes, nb in SHAPES[1:4]:
                got = H.thickness(m, types, lanes, nb)
                for name, g, w in zip(("thickness", "cover", "sections"), got, want):
                    assert R.same_bits(g, w), f"{dims} {types} lanes {lanes} workgroups {nb}: {name}"
        # each NULL combination of the outputs
        types = R.TYPE_LISTS[1]
        want = R.thickness(s, types)
        for mask in range(8):
            sel = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
            got = H.thickness(m, types, want=sel)
            for on, g, w in zip(sel, got, want):
                assert (g is None) if not on else R.same_bits(g, w)


def test_thickness_cover_takes_the_highest_section():
    s, m, _ = case((5, 7))
    th, cv, ns = R.thickness(s, [1, 2])
    c = 2                                        # pattern 2: A, B, A
    a = int(s.count[:c].sum())
    assert ns[0, c] == 2 and cv[0, c] == 0.0 and cv[1, c] == s.size[a + 2] and th[0, c] == s.size[a + 2] + s.size[a]
    assert th[0, 0] == 0.0 and cv[0, 0] == -1.0 and ns[0, 0] == 0 and not np.signbit(th[0, 0]), "an empty column"
    assert H.lib().sh_thickness(m.h, 64, 1, capi.ptr(np.array([1, 2, 1], np.uint32)), 3, None, None, None, None) == -2, "a repeated type"
    assert H.lib().sh_thickness(m.h, 64, 1, capi.ptr(np.arange(9, dtype=np.uint32)), 9, None, None, None, None) == -2


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_cores(dims):
    for s, m, _ in cases(dims):
        n = s.ncells
        rng = np.random.default_rng(n)
        lists = [np.arange(n), rng.integers(0, n, size=min(3 * n, 500)), np.array([n - 1, 0, n - 1, n - 1])]
        for cells in lists:
            want = R.cores(s, cells)
            for lanes, nb in SHAPES[1:4]:
                rc, total, *got = H.cores(m, cells, lanes, nb)
                assert rc == 0 and total == len(want[1])
                R.assert_same_cores(got, want, f"{dims} lanes {lanes} workgroups {nb}")
        # the whole map as one list is the snapshot
        rc, total, *got = H.cores(m, np.arange(n))
        R.assert_same_cores(got, (s.count, s.type, s.size, s.floor, s.sat), f"{dims}: the whole map")


def test_cores_cap_one_short_and_an_empty_list():
    s, m, _ = case((5, 7))
    cells = np.array([2, 3, 2, 0, 34])
    want = R.cores(s, cells)
    total = len(want[1])
    into = [np.full(total, 77, np.uint32), np.full(total, 77.0), np.full(total, 77.0), np.full(total, 77.0)]
    rc, tot, count, *arrs = H.cores(m, cells, cap=total - 1, into=into)
    assert rc == 1 and tot == total and (count == want[0]).all()
    assert all((a == 77).all() for a in arrs), "the section arrays stay untouched"
    rc, tot, count, *arrs = H.cores(m, cells, cap=total, into=into)
    assert rc == 0
    R.assert_same_cores((count, *arrs), want, "cap == total")
    t = C.c_uint64(9)
    assert H.lib().sh_cores(m.h, 64, 1, None, 0, None, 0, C.byref(t), None, None, None, None, None) == 0 and t.value == 0
    bad = C.c_uint64()
    assert H.lib().sh_cores(m.h, 64, 1, capi.ptr(np.array([1, 35], np.uint32)), 2, None, 0, C.byref(t), None, None, None, None, C.byref(bad)) == -2 and bad.value == 1


# ---------------------------------------------------------------- the committed goldens
ANCHORS = {
    ("default64", 20): {0: (399, 18910634942656), 1: (4096, 2669365980220864)},
    ("rgps64", 10): {1: (4096, 2288628419001724), 2: (60040, 37482512810019), 4: (60757, 90106993902542)},
    ("painted64", 5): {},
    ("rocksand48x80", 5): {},
}


@pytest.mark.parametrize("name,tick", sorted(ANCHORS), ids=lambda v: str(v))
def test_goldens(name, tick):
    s = golden_snapshot(name, tick)
    nt = min(s.nsoils, 64)
    want = R.totals(s, nt)
    for t, (sections, vol) in ANCHORS[(name, tick)].items():
        assert (want[0][t]["sections"], want[0][t]["volume_q40"]) == (sections, vol), f"type {t}"
    if name == "rgps64":
        for t in (0, 3):
            assert all(want[0][t][k] == 0 for k in ("sections", "cells", "top_cells", "volume_q40", "held_q40", "flags"))
        assert int(s.count.max()) == 893 and s.nsec == 124893, "the deep-column case"
        assert float(s.size[s.size > 0].min()) < 2.0 ** -40, "sections smaller than one unit are real"
    m = H.HostMap(s)
    for lanes, nb in SHAPES:
        R.assert_same_totals(H.totals(m, nt, lanes, nb), want, f"{name}.t{tick} lanes {lanes} workgroups {nb}")
    R.assert_same_totals(R.totals_np(s, nt), want, "the vectorised fold")
    assert sum(r["sections"] for r in want[0]) + want[1] == s.nsec and want[1] == 0
    assert want[0][0]["top_cells"] == figures_ref(s)["wet_cells"]
    for t, r in enumerate(want[0]):              # the one fact of the header: below the exact sum by less than sections * 2^-40
        exact = math.fsum(float(v) for v in s.size[s.type == t])
        assert r["flags"] == 0
        assert 0.0 <= exact - r["volume"] < r["sections"] * 2.0 ** -40 + math.ulp(exact) or r["sections"] == 0
    types = [t for t in R.TYPE_LISTS[1] if t < nt] or [0]
    wth = R.thickness(s, types)
    got = H.thickness(m, types, 256, 5)
    assert all(R.same_bits(g, w) for g, w in zip(got, wth))
    assert (wth[2].sum(axis=0) <= s.count).all()
    cells = np.arange(0, s.ncells, 37)
    rc, total, *cr = H.cores(m, cells, 64, 9)
    R.assert_same_cores(cr, R.cores(s, cells), f"{name}.t{tick} cores")


# ---------------------------------------------------------------- corrupt chains: host bodies only, never the device
def _untouched_calls(m, cell, what):
    out = (capi.SoilTotal * 64)()
    for r in out:
        r.sections = 12345
    other = np.full(1, 99, np.uint64)
    with pytest.raises(H.BadChain) as e:
        H.totals(m, 64, 64, 3, out=out, other=other)
    assert e.value.cell == cell, f"{what}: totals name cell {e.value.cell}"
    assert all(r.sections == 12345 for r in out) and other[0] == 99
    n = m.dimx * m.dimy
    into = [np.full((1, n), 5.0), np.full((1, n), 5.0), np.full((1, n), 5, np.uint32)]
    with pytest.raises(H.BadChain) as e:
        H.thickness(m, [1], 256, 2, into=into)
    assert e.value.cell == cell and all((a == 5).all() for a in into), f"{what}: thickness"
    arrs = [np.full(4096, 5, np.uint32), np.full(4096, 5.0), np.full(4096, 5.0), np.full(4096, 5.0)]
    with pytest.raises(H.BadChain) as e:
        H.cores(m, np.arange(n)[::-1], cap=4096, into=arrs)
    assert e.value.cell == cell and all((a == 5).all() for a in arrs), f"{what}: cores"


def test_corrupt_chains_return_minus_5_with_the_lowest_cell_and_write_nothing():
    s = R.synthetic((5, 7))
    # a prev beyond the pool, in two cells: the lower one is named
    m = H.HostMap(s)
    m.prev(14, value=m.pool_size)               # cell 14 (pattern 2) ...
    m.prev(26, value=0x7FFFFFFF)                # ... and cell 26 (pattern 2)
    _untouched_calls(m, 14, "beyond the pool")
    # a cycle: the bottom section of cell 8's column points back at the section under its top
    m = H.HostMap(s)
    first = m.prev(8)                           # (pattern 8: five sections)
    at = first
    while m.prev(at, pool=True) != 0xFFFFFFFF:
        at = m.prev(at, pool=True)
    m.prev(at, pool=True, value=first)
    _untouched_calls(m, 8, "a cycle")
    # members of an ensemble: the first bad member is named
    good, bad = H.HostMap(s), H.HostMap(s)
    bad.prev(3, value=bad.pool_size + 7)
    with pytest.raises(H.BadChain) as e:
        H.totals_many([good, bad, bad], 8)
    assert (e.value.member, e.value.cell) == (1, 3)


# ---------------------------------------------------------------- the transect rule
def test_transect_rule_in_the_eight_octants():
    T = Layermap.transect_cells
    assert T((4, 9), (4, 9)) == [(4, 9)], "N = 0 is the single cell"
    want = {
        (5, 2): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)],
        (2, 5): [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)],
    }
    for (dx, dy), pts in want.items():
        for sx in (1, -1):
            for sy in (1, -1):
                got = T((10, 20), (10 + sx * dx, 20 + sy * dy))
                assert got == [(10 + sx * x, 20 + sy * y) for x, y in pts], (dx, dy, sx, sy)
    assert T((0, 0), (3, 0)) == [(0, 0), (1, 0), (2, 0), (3, 0)] and T((0, 3), (0, 0)) == [(0, 3), (0, 2), (0, 1), (0, 0)]
    assert T((0, 0), (3, 3)) == [(i, i) for i in range(4)] and T((3, 0), (0, 3)) == [(3 - i, i) for i in range(4)]
    # the rule itself, and that consecutive points are neighbours, over a sweep of directions
    for x1 in range(-7, 8):
        for y1 in range(-7, 8):
            pts = T((0, 0), (x1, y1))
            n = max(abs(x1), abs(y1))
            assert len(pts) == n + 1 and pts[0] == (0, 0) and pts[-1] == (x1, y1)
            for i, (x, y) in enumerate(pts):
                if n:
                    assert x == int(np.sign(x1)) * ((2 * i * abs(x1) + n) // (2 * n)) and y == int(np.sign(y1)) * ((2 * i * abs(y1) + n) // (2 * n))
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(pts, pts[1:]))


# ---------------------------------------------------------------- the sanitizers over the stand-alone check
def test_strata_check_under_the_sanitizers(tmp_path):
    src = os.path.join(H.HERE, "strata_check.cpp")
    exe = str(tmp_path / "strata_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and "ok" in r.stdout
