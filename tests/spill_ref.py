"""Spill analysis restated in plain Python loops (include/soilmx.h, "spill analysis") on top of drainage_ref -- TEST INFRASTRUCTURE ONLY.

Heights are ordered by K = lakes_ref.key (-0 below +0, a positive NaN above +inf). A pass of basin a is (c, n): c in a, n an in-map
neighbour in another basin, w = max(h(c), h(n)); a border cell of a also has the off-map pass (c, NONE) with w = h(c). The pour point
is the pass with the smallest (K(w), c, n). The fill level L(a) = min over the passes of max(w, L(basin(n))), w itself off the map,
found here by Jacobi rounds from "no level yet": every round computes all levels from the levels of the round before. filled(c) =
max(h(c), L(basin(c))). storage_q40 = the sum over the basin's cells below the pour height of floor((pour_height - h) * 2^40),
fill_storage_q40 the same against the fill level. priority_flood() is an independent heap flood over the CELLS.
"""
from __future__ import annotations

import heapq
import math
import struct

import numpy as np

import drainage_ref as D
import lakes_ref as L
from soilmachine_amd.snapshot import Snapshot

NONE = 0xFFFFFFFF
F_LAKE, F_OFFMAP, F_NESTED, F_STORAGE, F_FILL_STORAGE = 1, 2, 4, 8, 16
FIELDS = ("first_cell", "pour_cell", "pour_to", "to_basin", "flags", "cells_below", "pour_height", "fill_height", "storage_q40", "fill_storage_q40")
FLOATS = ("pour_height", "fill_height")
TOP = 1 << 64                          # above every key: no level yet


def unkey(k: int) -> float:
    b = (k & 0x7FFFFFFFFFFFFFFF) if k >> 63 else (~k) & 0xFFFFFFFFFFFFFFFF
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def q40(d: float):
    """(floor(d * 2^40), unreliable?) of one cell below a level."""
    if not (d >= 0.0) or not (d < 16777216.0):
        return 0, True
    return int(math.floor(d * 1099511627776.0)), False


def spill(s: Snapshot, base=None):
    """(records, filled, extra): one dict per basin in the rank order of drainage_ref.drainage(s) (`base`: that result, where the
    caller has it); the (dimx, dimy) float64 plane; extra = {"rounds": Jacobi rounds, the final unchanged one included,
    "passes": the number of passes, "boundary": the number of cells that have one}."""
    dimx, dimy = int(s.dimx), int(s.dimy)
    n = dimx * dimy
    drecs, planes, _ = base if base is not None else D.drainage(s)
    lab = [int(v) for v in planes["labels"].reshape(n)]
    wet, h = D.heights(s)
    hl = [float(v) for v in h]
    K = [L.key(v) for v in hl]
    nb = len(drecs)
    passes = [[] for _ in range(nb)]          # per basin: (K(w), c, n, basin of n or -1)
    boundary = 0
    for c in range(n):
        a = lab[c]
        x, y = divmod(c, dimy)
        has = False
        for dx, dy in L.NB8:
            u, v = x + dx, y + dy
            if 0 <= u < dimx and 0 <= v < dimy:
                d = u * dimy + v
                if lab[d] != a:
                    passes[a].append((max(K[c], K[d]), c, d, lab[d]))
                    has = True
        if x in (0, dimx - 1) or y in (0, dimy - 1):
            passes[a].append((K[c], c, NONE, -1))
            has = True
        boundary += has
    pour = [min(p) for p in passes]           # (K(w), c, n, ...): lexicographic; (c, n) names a pass, so the rest never decides
    # the fill levels: Jacobi rounds over the cheapest pass per pair of basins
    edge = [{} for _ in range(nb)]
    for a in range(nb):
        for kw, c, d, b in passes[a]:
            if kw < edge[a].get(b, TOP):
                edge[a][b] = kw
    lev = [TOP] * nb
    rounds = 0
    todo = range(nb)                          # a basin none of whose neighbours changed in the round before keeps its level: skipped
    while True:
        rounds += 1
        new = {}
        for a in todo:
            best = lev[a]
            for b, kw in edge[a].items():
                k = kw if b < 0 else max(kw, lev[b])
                if k < best:
                    best = k
            if best < lev[a]:
                new[a] = best
        for a, k in new.items():               # (all of a round's levels come from the levels of the round before)
            lev[a] = k
        if not new:
            break
        todo = sorted({b for a in new for b in edge[a] if b >= 0})     # (passes are mutual: a's neighbours are the basins that see a)
    assert all(v < TOP for v in lev)
    recs = []
    acc = [[0, 0, 0, 0] for _ in range(nb)]   # storage, fill storage, cells below, flags
    filled = np.zeros(n)
    for c in range(n):
        a = lab[c]
        kp, kl = pour[a][0], lev[a]
        if K[c] < kp:
            q, bad = q40(unkey(kp) - hl[c])
            acc[a][0] += q
            acc[a][2] += 1
            if bad:
                acc[a][3] |= F_STORAGE
        if K[c] < kl:
            q, bad = q40(unkey(kl) - hl[c])
            acc[a][1] += q
            if bad:
                acc[a][3] |= F_FILL_STORAGE
        filled[c] = unkey(max(K[c], kl))
    for a in range(nb):
        kw, c, d, b = pour[a]
        st, fs, below, flags = acc[a]
        if st >= TOP:
            flags |= F_STORAGE
        if fs >= TOP:
            flags |= F_FILL_STORAGE
        if drecs[a]["flags"] & D.F_LAKE:
            flags |= F_LAKE
        if d == NONE:
            flags |= F_OFFMAP
        if lev[a] > kw:
            flags |= F_NESTED
        recs.append({"first_cell": drecs[a]["first_cell"], "pour_cell": c, "pour_to": d, "to_basin": NONE if d == NONE else drecs[b]["first_cell"], "flags": flags,
                     "cells_below": below, "pour_height": unkey(kw), "fill_height": unkey(lev[a]), "storage_q40": st % TOP, "fill_storage_q40": fs % TOP})
    return recs, filled.reshape(dimx, dimy), {"rounds": rounds, "passes": sum(len(p) for p in passes), "boundary": boundary}


def priority_flood(s: Snapshot) -> np.ndarray:
    """The minimax height (by K) over 8-connected cell paths from each cell to off the map, the cell's own height included: a heap
    flood from the border inwards. Knows nothing of basins or lakes."""
    dimx, dimy = int(s.dimx), int(s.dimy)
    n = dimx * dimy
    _, h = D.heights(s)
    K = [L.key(float(v)) for v in h]
    out = [None] * n
    heap = []
    for c in range(n):
        x, y = divmod(c, dimy)
        if x in (0, dimx - 1) or y in (0, dimy - 1):
            out[c] = K[c]
            heap.append((K[c], c))
    heapq.heapify(heap)
    while heap:
        k, c = heapq.heappop(heap)
        if k != out[c]:
            continue
        x, y = divmod(c, dimy)
        for dx, dy in L.NB8:
            u, v = x + dx, y + dy
            if 0 <= u < dimx and 0 <= v < dimy:
                d = u * dimy + v
                kd = max(K[d], k)
                if out[d] is None or kd < out[d]:
                    out[d] = kd
                    heapq.heappush(heap, (kd, d))
    return np.array([unkey(k) for k in out]).reshape(dimx, dimy)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def keys(a) -> list:
    return [L.key(float(v)) for v in np.asarray(a, np.float64).reshape(-1)]


def same(a: dict, b: dict) -> list:
    """Field-by-field comparison of two records, floats by their bits; the list of differing fields."""
    bad = []
    for f in FIELDS:
        u, v = a[f], b[f]
        if f in FLOATS:
            if L.bits(u) != L.bits(v):
                bad.append(f"{f}: {u!r} vs {v!r}")
        elif int(u) != int(v):
            bad.append(f"{f}: {u} vs {v}")
    return bad


def assert_same_spill(got, want, what="", count=None):
    """got / want = (records, filled or None, ...)."""
    gr, gf, wr, wf = got[0], got[1], want[0], want[1]
    if count is not None:
        assert count == len(wr), f"{what}: {count} basins counted, expected {len(wr)}"
    assert len(gr) == len(wr), f"{what}: {len(gr)} records, expected {len(wr)}"
    for k, (a, b) in enumerate(zip(gr, wr)):
        bad = same(a, b)
        assert not bad, f"{what}: basin {k}: " + "; ".join(bad)
    if gf is not None and wf is not None:
        g, w = bits(gf).reshape(-1), bits(wf).reshape(-1)
        assert np.array_equal(g, w), f"{what}: the filled planes differ at {int((g != w).sum())} cells, the first at cell {int(np.flatnonzero(g != w)[0])}"


def assert_invariants(name, recs, drecs, what=""):
    """What holds for every map: the records are the basins of drainage(), one for one; the fill level is never below the pour
    height; a basin that pours off the map pours into no basin, every other one into another basin; some basin pours off the map.
    The last one the definitions themselves rule out on a map of ONE height -- `plateau`: every cell is a basin, every pass has the
    cell's height, and at an equal height an in-map neighbour beats the off-map pass. There every basin pours, and fills, at the
    common height, which is the height of its off-map passes too."""
    assert [r["first_cell"] for r in recs] == [r["first_cell"] for r in drecs], f"{what}: the records do not align with the basins of drainage()"
    first = {r["first_cell"] for r in recs}
    for r, b in zip(recs, drecs):
        assert L.key(r["fill_height"]) >= L.key(r["pour_height"]), f"{what}: basin {r['first_cell']} fills below its pour height"
        assert bool(r["flags"] & F_NESTED) == (L.key(r["fill_height"]) > L.key(r["pour_height"]))
        assert bool(r["flags"] & F_LAKE) == bool(b["flags"] & D.F_LAKE), f"{what}: basin {r['first_cell']}: the lake bit"
        if r["flags"] & F_OFFMAP:
            assert r["to_basin"] == NONE and r["pour_to"] == NONE, f"{what}: basin {r['first_cell']} pours off the map and into a basin"
        else:
            assert r["to_basin"] in first and r["to_basin"] != r["first_cell"] and r["pour_to"] != NONE, f"{what}: basin {r['first_cell']}: to_basin"
        assert r["cells_below"] <= b["cells"] and (r["cells_below"] > 0 or r["storage_q40"] == 0)
    if name != "plateau":
        assert any(r["flags"] & F_OFFMAP for r in recs), f"{what}: no basin pours off the map"
    else:
        assert not any(r["flags"] & (F_OFFMAP | F_NESTED) for r in recs)
        assert all(L.bits(r["pour_height"]) == L.bits(1.0) and L.bits(r["fill_height"]) == L.bits(1.0) for r in recs)


# ---- the inputs added to drainage_ref.INPUTS ----
def _jitter(dx, dy, scale=2.0 ** -24):
    return (np.arange(dx * dy) * scale).reshape(dx, dy)


def _border_distance(dx, dy):
    x, y = np.indices((dx, dy))
    return np.minimum(np.minimum(x, dx - 1 - x), np.minimum(y, dy - 1 - y))


def i_nested(dx, dy):
    """A bowl inside a bowl. From the border inwards: two rings of a thick outer rim (10, 9), a moat (5), the inner bowl's rim (7),
    the inner bowl (falling from 3 to its middle). The inner bowl pours over its rim into the moat, the moat cannot leave below 9:
    the inner bowl's fill level lies above its pour height (flag 4). One border cell is a pit in the rim (8): it pours off the map."""
    d = _border_distance(dx, dy)
    level = np.select([d == 0, d == 1, d == 2, d == 3], [10.0, 9.0, 5.0, 7.0], 3.0 - 0.01 * d)
    h = level + _jitter(dx, dy)
    if dx > 2:
        h[dx // 2, 0] = 8.0
    return D._snap(dx, dy, h)


def rim_notch(dx, dy):
    return (0, dy // 2)


def i_rim(dx, dy):
    """A high border (4, and 3 one ring further in) around random heights below 1; one notch: the border cell rim_notch at 2, the
    cell behind it at 2.5. The notch is a sink of its own that pours off the map; everything inside leaves through it, at 2.5."""
    d = _border_distance(dx, dy)
    inner = D.perm_heights(np.random.default_rng(31).permutation(dx * dy)).reshape(dx, dy) / max(1.0, dx * dy * 2.0 ** -10)
    h = np.select([d == 0, d == 1], [4.0 + _jitter(dx, dy), 3.0 + _jitter(dx, dy)], inner)
    x, y = rim_notch(dx, dy)
    h[x, y] = 2.0
    if dx > 1:
        h[x + 1, y] = 2.5
    return D._snap(dx, dy, h)


LAKE_LEVEL = 1.5


def lake_box(dx, dy):
    return dx // 4, (3 * dx) // 4, dy // 8, (7 * dy) // 8


def i_level_lake(dx, dy):
    """A levelled lake (every wet cell's floor + size is exactly 1.5) over a rough bed, wide enough to cross the edges of every tile
    shape; dry land from 2 upwards around it, so the lake has freeboard."""
    x0, x1, y0, y1 = lake_box(dx, dy)
    wet = np.zeros((dx, dy), bool)
    wet[x0:x1, y0:y1] = True
    k = np.random.default_rng(32).permutation(dx * dy).reshape(dx, dy)
    bed = (k % 512) * 2.0 ** -10                            # below 0.5, exact
    land = 2.0 + k * 2.0 ** -10
    return L.make_snapshot(wet, LAKE_LEVEL - bed, np.where(wet, bed, land))


def chain_layout(dx, dy):
    """(pit columns, first column) of i_chain, or None where the map is too small for it."""
    if dy < 7:
        return None
    per = (dy - 2) // 2
    p = -(-64 // per)
    x0 = dx - 2 - (4 * p - 4)
    return (p, x0) if x0 >= 2 else None


def i_chain(dx, dy):
    """At least 64 basins in series behind a rim. One-cell corridors between one-cell walls (100) at the right end of the map: a PIT
    column is walked towards larger y and alternates pits (0.25) and ridges (1); a connector (1) leads to a RETURN column, a slope
    walked back towards smaller y (one basin), and on to the next pit column. The last pit column is x = dimx - 2; the corner cell
    dimx*dimy - 1 (0.5) is the only way out below the rim. Along the chain towards the outlet the cell index only grows inside the pit
    columns, so a sweep over the cells in ascending order carries the level back one basin only. The rest of the map slopes away to x = 0."""
    lay = chain_layout(dx, dy)
    if lay is None:
        return D.i_ramp_x(dx, dy)
    p, xs = lay
    x, y = np.indices((dx, dy))
    h = 100.0 + _jitter(dx, dy, 2.0 ** -20)
    left = x < xs - 1
    h[left] = (150.0 + x + y * 2.0 ** -10)[left]
    for k in range(p):
        xp = xs + 4 * k
        for yy in range(1, dy - 1):
            h[xp, yy] = 0.25 if (yy - 1) % 2 == 0 else 1.0
        if k + 1 < p:
            h[xp + 1, dy - 2] = 1.0                          # the connector at the far end
            for yy in range(1, dy - 1):
                h[xp + 2, yy] = 0.3 + 0.5 * yy / dy          # the return slope: falls towards y = 1
            h[xp + 3, 1] = 1.0                               # the connector back
    h[dx - 1, dy - 1] = 0.5
    return D._snap(dx, dy, h)


def unreliable_cells(dx, dy):
    """(the deep pit, the sink inside the NaN ring, the ring)"""
    pit = ((3 * dx) // 4) * dy + (3 * dy) // 4
    sx, sy = dx // 4, dy // 4
    ring = [u * dy + v for u in range(sx - 1, sx + 2) for v in range(sy - 1, sy + 2) if (u, v) != (sx, sy) and 0 <= u < dx and 0 <= v < dy]
    return pit, sx * dy + sy, ring


def i_unreliable(dx, dy):
    """Random heights in [1, 2); one pit 2^25 deep (its difference to any level is >= 2^24) and one sink whose neighbours are all
    NaN: its pour height and its fill level are NaN, the difference is not finite."""
    h = 1.0 + D.perm_heights(np.random.default_rng(33).permutation(dx * dy)) / max(1.0, dx * dy * 2.0 ** -10)
    pit, sink, ring = unreliable_cells(dx, dy)
    h[pit] = -33554432.0
    h[sink] = 0.5
    h[ring] = np.nan
    return D._snap(dx, dy, h)


NEW_INPUTS = {"nested": i_nested, "rim": i_rim, "level_lake": i_level_lake, "chain": i_chain, "unreliable": i_unreliable}
INPUTS = dict(D.INPUTS, **NEW_INPUTS)
SIZES = D.SIZES
BIG = D.BIG
DRY_INPUTS = ("cone", "ramp_x", "ramp_y", "spiral", "plateau", "ties", "corners")     # filled == the priority flood, bit for bit

_cases = {}


def case(name: str, dims: tuple):
    """(snapshot, drainage, spill) of an input, computed once and shared by the tests that need it."""
    k = (name, tuple(dims))
    if k not in _cases:
        if name in D.INPUTS:
            s, base = D.case(name, dims)
        else:
            s = INPUTS[name](*dims)
            base = D.drainage(s)
        _cases[k] = (s, base, spill(s, base))
    return _cases[k]


def all_cases():
    """Every input at every size, 128 x 128 included."""
    return [(n, d) for d in SIZES + [BIG] for n in sorted(INPUTS)]
