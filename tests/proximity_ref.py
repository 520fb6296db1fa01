"""Proximity restated in numpy and plain Python (include/soilmx.h, "proximity") -- TEST INFRASTRUCTURE ONLY.

For every cell the minimum of d2 * 2^32 + site over ALL sites, in chunks of cells: no separable trick, no envelope. The records and
the buffer rows are folded from the planes by plain loops in cell order. In WATER mode the sites are the wet cells and their groups
the lake ranks of tests/lakes_ref.py.
"""
from __future__ import annotations

import math

import numpy as np

import lakes_ref

NONE = 0xFFFFFFFF
F_BORDER = 1
FIELDS = ("site", "sites", "cells", "dist2_max", "farthest_cell", "flags", "dist2_sum", "x0", "y0", "x1", "y1")
PLANES = ("nearest", "group", "dist2")
SIZES = list(lakes_ref.SIZES) + [(128, 128)]


# ---- the site patterns: masks as functions of (dx, dy) ----
def p_none(dx, dy):
    return np.zeros((dx, dy), bool)


def p_all(dx, dy):
    return np.ones((dx, dy), bool)


def p_corner(dx, dy):
    m = np.zeros((dx, dy), bool)
    m[0, 0] = True
    return m


def p_last(dx, dy):
    m = np.zeros((dx, dy), bool)
    m[dx - 1, dy - 1] = True
    return m


def p_row(dx, dy):
    """One full row: the cells of equal y."""
    m = np.zeros((dx, dy), bool)
    m[:, dy // 2] = True
    return m


def p_column(dx, dy):
    m = np.zeros((dx, dy), bool)
    m[dx // 3, :] = True
    return m


def p_last_column(dx, dy):
    """One site, in the last column: every envelope has one entry, pushed at the last step."""
    m = np.zeros((dx, dy), bool)
    m[dx - 1, dy // 2] = True
    return m


def p_column_pair(dx, dy):
    """Two sites two cells apart in one column: the cell between them ties inside the column (the smaller row wins)."""
    m = np.zeros((dx, dy), bool)
    x, y = dx // 2, max(0, dy // 2 - 1)
    m[x, y] = True
    m[x, min(dy - 1, y + 2)] = True
    return m


def p_mirror(dx, dy):
    """Two sites mirrored across the main diagonal: every diagonal cell ties across columns (the smaller column wins)."""
    m = np.zeros((dx, dy), bool)
    a, b = min(dx, dy) // 4, min(dx, dy) // 2
    m[min(a, dx - 1), min(b, dy - 1)] = True
    m[min(b, dx - 1), min(a, dy - 1)] = True
    return m


def p_checker(dx, dy):
    x, y = np.indices((dx, dy))
    return (x + y) % 2 == 0


def p_bernoulli(p, seed):
    def f(dx, dy):
        m = np.random.default_rng(seed).random((dx, dy)) < p
        if not m.any():
            m[dx // 2, dy // 2] = True
        return m
    return f


PATTERNS = {
    "none": p_none, "all": p_all, "corner": p_corner, "last": p_last, "row": p_row, "column": p_column, "last_column": p_last_column,
    "column_pair": p_column_pair, "mirror": p_mirror, "checker": p_checker, "bernoulli20": p_bernoulli(0.2, 2024), "bernoulli1": p_bernoulli(0.01, 99),
}
LARGE = ("corner", "mirror", "row", "bernoulli1", "bernoulli20")      # the five inputs the device runs at 128 x 128


def site_list(name: str, dims: tuple) -> np.ndarray:
    """The pattern's sites as a list, in DESCENDING cell order: a list position is not the rank of the cell."""
    return np.ascontiguousarray(np.flatnonzero(PATTERNS[name](*dims).reshape(-1))[::-1], np.uint32)


# ---- the planes ----
def planes_of(dimx: int, dimy: int, sites, groups) -> dict:
    """nearest, group and dist2 as (dimx, dimy) uint32 planes. sites: cell indices; groups: the group of each."""
    n = dimx * dimy
    sites = np.asarray(sites, np.int64).reshape(-1)
    groups = np.asarray(groups, np.uint32).reshape(-1)
    out = {k: np.full(n, NONE, np.uint32) for k in PLANES}
    if sites.size:
        assert 2 * max(dimx, dimy) ** 2 < 2 ** 31 and n <= 2 ** 32
        order = np.argsort(sites)
        sites, groups = sites[order], groups[order]
        sx, sy = np.divmod(sites, dimy)
        chunk = max(1, (1 << 22) // sites.size)
        for at in range(0, n, chunk):
            c = np.arange(at, min(n, at + chunk), dtype=np.int64)
            cx, cy = np.divmod(c, dimy)
            d2 = (cx[:, None] - sx[None, :]) ** 2 + (cy[:, None] - sy[None, :]) ** 2
            key = (d2.astype(np.uint64) << np.uint64(32)) | sites.astype(np.uint64)[None, :]
            j = np.argmin(key, axis=1)
            out["nearest"][c] = sites[j]
            out["dist2"][c] = d2[np.arange(c.size), j]
            out["group"][c] = groups[j]
    return {k: v.reshape(dimx, dimy) for k, v in out.items()}


def root(d: int) -> int:
    """r with r^2 <= d < (r+1)^2. The f64 square root is exact for an integer below 2^52 up to its last bit, which cannot carry it
    over an integer: asserted against the integer root."""
    assert 0 <= d < 2 ** 52
    r = math.isqrt(d)
    assert int(math.sqrt(float(d))) == r
    return r


def fold(dimx: int, dimy: int, planes: dict, ngroups: int, bins: int = 0, bin_width: int = 1) -> list:
    """The records of groups 0 .. ngroups - 1 from the planes, cell after cell; with bins each gets its ``buffers`` row."""
    recs = [{"site": NONE, "sites": 0, "cells": 0, "dist2_max": 0, "farthest_cell": NONE, "flags": 0, "dist2_sum": 0, "x0": 0xFFFF, "y0": 0xFFFF, "x1": 0, "y1": 0}
            for _ in range(ngroups)]
    rows = np.zeros((ngroups, bins), np.uint32)
    gr, d2 = planes["group"].reshape(-1), planes["dist2"].reshape(-1)
    for c in range(dimx * dimy):
        g = int(gr[c])
        if g >= ngroups:
            continue
        r, d = recs[g], int(d2[c])
        x, y = divmod(c, dimy)
        if d == 0:
            r["sites"] += 1
            r["site"] = min(r["site"], c)
        if r["cells"] == 0 or d > r["dist2_max"]:
            r["dist2_max"], r["farthest_cell"] = d, c
        r["cells"] += 1
        r["dist2_sum"] += d
        if x == 0 or y == 0 or x == dimx - 1 or y == dimy - 1:
            r["flags"] |= F_BORDER
        r["x0"], r["x1"], r["y0"], r["y1"] = min(r["x0"], x), max(r["x1"], x), min(r["y0"], y), max(r["y1"], y)
        if bins:
            rows[g, min(root(d) // bin_width, bins - 1)] += 1
    for g, r in enumerate(recs if bins else ()):
        r["buffers"] = rows[g].copy()
    return recs


def proximity(dimx: int, dimy: int, cells=None, snapshot=None, bins: int = 0, bin_width: int = 1, cap: int | None = None):
    """(records, planes, nrecords). cells: the list (LIST mode); None: the wet cells of `snapshot` (WATER mode), at most `cap` records."""
    if cells is not None:
        cells = np.asarray(cells, np.int64).reshape(-1)
        assert cells.size and len(set(cells.tolist())) == cells.size and cells.min() >= 0 and cells.max() < dimx * dimy
        pl = planes_of(dimx, dimy, cells, np.arange(cells.size))
        n = cells.size
    else:
        lakes, labels = lakes_ref.census(snapshot)
        lab = labels.reshape(-1)
        wet = np.flatnonzero(lab != lakes_ref.DRY)
        pl = planes_of(dimx, dimy, wet, lab[wet])
        n = len(lakes)
    recs = fold(dimx, dimy, pl, n if cap is None else min(n, cap), bins, bin_width)
    if cells is not None:
        assert [r["site"] for r in recs] == cells.tolist() and all(r["sites"] == 1 for r in recs)
    else:
        assert all(r["site"] == k["first_cell"] and r["sites"] == k["cells"] for r, k in zip(recs, lakes))
    return recs, pl, n


_cases = {}


def case(name: str, dims: tuple, bins: int = 0, bin_width: int = 1):
    """(list, (records, planes, nrecords)) of a pattern in LIST mode, computed once and shared by the tests that need it; the pattern
    without a site has no list: (None, None)."""
    k = (name, tuple(dims), bins, bin_width)
    if k not in _cases:
        cl = site_list(name, dims)
        _cases[k] = (cl, proximity(dims[0], dims[1], cl, bins=bins, bin_width=bin_width)) if cl.size else (None, None)
    return _cases[k]


_water = {}


def water_case(name: str, dims: tuple, bins: int = 0, bin_width: int = 1):
    """(snapshot, (records, planes, nrecords)) of a wet mask of tests/lakes_ref.py in WATER mode, computed once."""
    k = (name, tuple(dims), bins, bin_width)
    if k not in _water:
        s = lakes_ref.case(name, dims)[0]
        _water[k] = (s, proximity(dims[0], dims[1], snapshot=s, bins=bins, bin_width=bin_width))
    return _water[k]


# ---- comparisons ----
def assert_same_proximity(got, want, what="", planes=PLANES):
    """got / want = (records, planes, nrecords): every field, every row and every plane that `got` holds."""
    (gr, gp, gn), (wr, wp, wn) = got, want
    assert gn == wn, f"{what}: {gn} records counted, expected {wn}"
    assert len(gr) == len(wr), f"{what}: {len(gr)} records, expected {len(wr)}"
    for k, (a, b) in enumerate(zip(gr, wr)):
        bad = [f"{f}: {a[f]} vs {b[f]}" for f in FIELDS if int(a[f]) != int(b[f])]
        assert not bad, f"{what}: record {k}: " + "; ".join(bad)
        assert ("buffers" in a) == ("buffers" in b), f"{what}: record {k}: buffers"
        if "buffers" in b:
            assert np.array_equal(np.asarray(a["buffers"], np.uint32), b["buffers"]), f"{what}: record {k}: buffers {a['buffers']} vs {b['buffers']}"
    for p in planes:
        if gp is not None and p in gp:
            assert np.array_equal(np.asarray(gp[p], np.uint32).reshape(wp[p].shape), wp[p]), f"{what}: the {p} planes differ"


def assert_invariants(dimx: int, dimy: int, result, sites, transposed=None, what=""):
    """What holds for every result with all its records and planes. sites: the site cells; transposed: the planes of the transposed
    map with the transposed sites (any list order), where the caller has them."""
    recs, pl, n = result
    near, gr, d2 = (pl[k].astype(np.int64) for k in PLANES)
    sites = np.asarray(sites, np.int64).reshape(-1)
    if sites.size == 0:
        assert n == 0 and not recs and (near == NONE).all() and (gr == NONE).all() and (d2 == NONE).all(), f"{what}: a map without a site"
        return
    if len(recs) == n:
        assert sum(r["cells"] for r in recs) == dimx * dimy, f"{what}: the zones do not partition the map"
    flat = near.reshape(-1)
    assert np.array_equal(flat[sites], sites) and (d2.reshape(-1)[sites] == 0).all(), f"{what}: a site is not its own nearest"
    assert np.isin(flat, sites).all(), f"{what}: a nearest that is no site"
    cx, cy = np.indices((dimx, dimy))
    assert np.array_equal((cx - near // dimy) ** 2 + (cy - near % dimy) ** 2, d2), f"{what}: dist2 is not the distance to nearest"
    assert np.array_equal(gr, gr.reshape(-1)[flat].reshape(dimx, dimy)), f"{what}: group is not the group of nearest"
    bound = 2.0 * np.sqrt(d2) + 1.0                     # |d(a) - d(b)| <= 1 between 4-neighbours, squared
    for a, b, ba, bb in ((d2[1:], d2[:-1], bound[1:], bound[:-1]), (d2[:, 1:], d2[:, :-1], bound[:, 1:], bound[:, :-1])):
        assert (a - b <= bb).all() and (b - a <= ba).all(), f"{what}: dist2 jumps between 4-neighbours"
    if transposed is not None:
        tn, td = transposed["nearest"].astype(np.int64), transposed["dist2"].astype(np.int64)
        assert np.array_equal(td.T, d2), f"{what}: the transposed map's dist2 is not the transpose"
        back = (tn % dimx) * dimy + tn // dimx           # the transposed map's nearest as a cell of this map: equally far, maybe another of a tie
        assert np.isin(back, sites).all(), f"{what}: the transposed map's nearest is no site"
        assert np.array_equal((cx - back.T // dimy) ** 2 + (cy - back.T % dimy) ** 2, d2), f"{what}: the transposed map's nearest is not as near"
    for k, r in enumerate(recs):
        if "buffers" in r:
            assert int(np.asarray(r["buffers"], np.int64).sum()) == r["cells"], f"{what}: row {k} does not sum to cells"


def transposed_sites(dimx: int, dimy: int, cells) -> np.ndarray:
    """The list's cells in the transposed (dimy, dimx) map."""
    c = np.asarray(cells, np.int64)
    return np.ascontiguousarray((c % dimy) * dimx + c // dimy, np.uint32)
