"""The sediment budget restated in plain Python loops over two ``Snapshot``s (include/soilmx.h, "the sediment budget") -- TEST
INFRASTRUCTURE ONLY. It owes nothing to soil_budget.h: Python integers for the q40 sums, Python floats for the two subtractions, the
basins from drainage_ref on the base. Also the synthetic pairs the CPU and the GPU tests share and the vectorised fold (two exports +
numpy) that tools/budget_bench.py times as what a caller had before.
"""
from __future__ import annotations

import numpy as np

import drainage_ref as D
import strata_ref as S
from soilmachine_amd.snapshot import Snapshot

EMPTY = NONE = 0xFFFFFFFF
F_TERM, F_WRAP, F_NAN = 1, 2, 4
M64 = (1 << 64) - 1
BASIN_FIELDS = ("first_cell", "cells", "lowered_cells", "raised_cells", "resurfaced_cells", "flags", "eroded_q40", "deposited_q40", "water_gained_q40",
                "water_lost_q40", "cut_max", "fill_max", "cut_cell", "fill_cell")
SOIL_FIELDS = ("gained_q40", "lost_q40", "held_gained_q40", "held_lost_q40", "cells_gained", "cells_lost", "surfaced", "covered", "flags")
PLANES = {"dground": np.float64, "dheight": np.float64, "dsolid": np.int64, "dwater": np.int64}


def _signed(v: int) -> int:
    """(int64) of a difference of two u64"""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def cells_of(s: Snapshot) -> list:
    """Per cell: top type (EMPTY for an empty column), ground, h, {type: [V, H, flags]}, S, the flags the cell gives its basin."""
    start, end = S._columns(s)
    ty, size, floor, sat = s.type.tolist(), s.size.tolist(), s.floor.tolist(), s.sat.tolist()
    out = []
    for c in range(s.ncells):
        a, b = int(start[c]), int(end[c])
        if a == b:
            out.append((EMPTY, 0.0, 0.0, {}, 0, 0))
            continue
        t = b - 1
        ground = floor[t] if ty[t] == 0 else floor[t] + size[t]
        per, solid, fb = {}, 0, 0
        for k in range(a, b):
            r = per.setdefault(ty[k], [0, 0, 0])
            q, ok = S._q40(size[k])
            r[0] += q
            if ty[k] != 0:
                solid += q
            if not ok:
                r[2] |= F_TERM
                fb |= F_TERM
            q, ok = S._q40(size[k] * sat[k])
            r[1] += q
            if not ok:
                r[2] |= F_TERM
        for k, r in per.items():
            if r[0] > M64 or r[1] > M64:
                r[2] |= F_WRAP
            if k == 0 and r[0] > M64:
                fb |= F_WRAP
            r[0] &= M64
            r[1] &= M64
        if solid > M64:
            fb |= F_WRAP
        out.append((ty[t], ground, floor[t] + size[t], per, solid & M64, fb))
    return out


def budget(base: Snapshot, now: Snapshot, ntypes: int, drain=None):
    """(basins, soils, planes) of base -> now: one dict per basin of the base's drainage in rank order, one per type < ntypes, the four
    (dimx, dimy) planes. drain: drainage_ref.drainage(base), where the caller has it."""
    assert (base.dimx, base.dimy) == (now.dimx, now.dimy)
    n = base.ncells
    drain = D.drainage(base) if drain is None else drain
    lab = np.asarray(drain[1]["labels"]).reshape(n).tolist()
    nb = len(drain[0])
    basins = [{"first_cell": drain[0][k]["first_cell"], "cells": drain[0][k]["cells"], "lowered_cells": 0, "raised_cells": 0, "resurfaced_cells": 0, "flags": 0, "eroded_q40": 0,
               "deposited_q40": 0, "water_gained_q40": 0, "water_lost_q40": 0, "cut_max": 0.0, "fill_max": 0.0, "cut_cell": NONE, "fill_cell": NONE} for k in range(nb)]
    soils = [{k: 0 for k in SOIL_FIELDS} for _ in range(ntypes)]
    dground, dheight = np.zeros(n), np.zeros(n)
    dsolid, dwater = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cb, cn = cells_of(base), cells_of(now)
    for c in range(n):
        tb, gb, hb, pb, sb, fb = cb[c]
        tn, gn, hn, pn, sn, fn = cn[c]
        wb, wn = pb.get(0, (0, 0, 0))[0], pn.get(0, (0, 0, 0))[0]
        dg = gn - gb
        dground[c], dheight[c] = dg, hn - hb
        dsolid[c], dwater[c] = _signed(sn - sb), _signed(wn - wb)
        r = basins[lab[c]]
        r["flags"] |= fb | fn | (F_NAN if (gn != gn or gb != gb) else 0)
        if gn < gb:
            r["lowered_cells"] += 1
            if -dg > r["cut_max"]:             # (cells in ascending order: the first to attain the extreme stays)
                r["cut_max"], r["cut_cell"] = -dg, c
        if gn > gb:
            r["raised_cells"] += 1
            if dg > r["fill_max"]:
                r["fill_max"], r["fill_cell"] = dg, c
        if tn != tb:
            r["resurfaced_cells"] += 1
            if tn < ntypes:
                soils[tn]["surfaced"] += 1
            if tb < ntypes:
                soils[tb]["covered"] += 1
        if sb > sn:
            r["eroded_q40"] += sb - sn
        if sn > sb:
            r["deposited_q40"] += sn - sb
        if wn > wb:
            r["water_gained_q40"] += wn - wb
        if wb > wn:
            r["water_lost_q40"] += wb - wn
        for t in set(pb) | set(pn):
            if t >= ntypes:
                continue
            (vb, xb, f0), (vn, xn, f1) = pb.get(t, (0, 0, 0)), pn.get(t, (0, 0, 0))
            q = soils[t]
            q["flags"] |= f0 | f1
            if vn > vb:
                q["gained_q40"] += vn - vb
                q["cells_gained"] += 1
            if vn < vb:
                q["lost_q40"] += vb - vn
                q["cells_lost"] += 1
            if xn > xb:
                q["held_gained_q40"] += xn - xb
            if xn < xb:
                q["held_lost_q40"] += xb - xn
    for r, keys in [(r, ("eroded_q40", "deposited_q40", "water_gained_q40", "water_lost_q40")) for r in basins] + \
                   [(q, ("gained_q40", "lost_q40", "held_gained_q40", "held_lost_q40")) for q in soils]:
        for k in keys:
            if r[k] > M64:
                r["flags"] |= F_WRAP
            r[k] &= M64
    for r in basins:
        r["eroded"], r["deposited"] = r["eroded_q40"] / 2 ** 40, r["deposited_q40"] / 2 ** 40
        r["net"] = (r["deposited_q40"] - r["eroded_q40"]) / 2 ** 40
    shape = (base.dimx, base.dimy)
    return basins, soils, {"dground": dground.reshape(shape), "dheight": dheight.reshape(shape), "dsolid": dsolid.reshape(shape), "dwater": dwater.reshape(shape)}


def assert_same_budget(got, want, what="", count=None, cap=None):
    """got / want = (basins, soils[, planes]); floats by their bits. cap: got holds the first cap basins only. A plane got lacks is
    not compared."""
    gb, gs, wb, ws = got[0], got[1], want[0], want[1]
    if count is not None:
        assert count == len(wb), f"{what}: {count} basins counted, expected {len(wb)}"
    wb = wb if cap is None else wb[:cap]
    assert len(gb) == len(wb), f"{what}: {len(gb)} basins, expected {len(wb)}"
    for k, (a, b) in enumerate(zip(gb, wb)):
        for f in BASIN_FIELDS:
            if f in ("cut_max", "fill_max"):
                assert S.bits(a[f]) == S.bits(b[f]), f"{what}: basin {k} {f}: {a[f]!r}, expected {b[f]!r}"
            else:
                assert int(a[f]) == int(b[f]), f"{what}: basin {k} {f}: {a[f]}, expected {b[f]}"
    if gs is not None:
        assert len(gs) == len(ws), f"{what}: {len(gs)} soil records, expected {len(ws)}"
        for t, (a, b) in enumerate(zip(gs, ws)):
            for f in SOIL_FIELDS:
                assert int(a[f]) == int(b[f]), f"{what}: soil {t} {f}: {a[f]}, expected {b[f]}"
    gp = got[2] if len(got) > 2 and got[2] else {}
    for p, g in gp.items():
        w = want[2][p]
        g = np.asarray(g).reshape(w.shape)
        assert g.dtype == w.dtype and S.same_bits(g, w), f"{what}: the {p} planes differ, the first at cell {int(np.flatnonzero(g.view(np.uint64).ravel() != w.view(np.uint64).ravel())[0])}"


def assert_invariants(base: Snapshot, now: Snapshot, basins, soils, planes=None, what=""):
    """What holds for every pair. `soils` must cover every type of both maps for 2; planes (all four) for 4."""
    n = base.ncells
    assert sum(r["cells"] for r in basins) == n, f"{what}: the basins' cells do not sum to the map"
    nt = len(soils)
    covered = int(max(base.type.max(initial=0), now.type.max(initial=0))) < nt
    clean = not any(r["flags"] & F_WRAP for r in basins) and not any(q["flags"] & F_WRAP for q in soils)   # (an unreliable term is 0 everywhere)
    if covered and clean:
        net = sum(r["deposited_q40"] - r["eroded_q40"] for r in basins)
        assert net == sum(q["gained_q40"] - q["lost_q40"] for q in soils[1:]), f"{what}: the basins' net is not the soils' net"
    if clean:
        tb, tn = S.totals(base, nt)[0], S.totals(now, nt)[0]
        for t, q in enumerate(soils):
            assert q["gained_q40"] - q["lost_q40"] == tn[t]["volume_q40"] - tb[t]["volume_q40"], f"{what}: soil {t}: gained - lost is not the change of the total"
            assert q["held_gained_q40"] - q["held_lost_q40"] == tn[t]["held_q40"] - tb[t]["held_q40"], f"{what}: soil {t}: the held change"
            assert q["surfaced"] - q["covered"] == tn[t]["top_cells"] - tb[t]["top_cells"], f"{what}: soil {t}: surfaced - covered is not the change of top_cells"
    if planes:
        dg = np.asarray(planes["dground"]).ravel()
        with np.errstate(invalid="ignore"):
            assert sum(r["lowered_cells"] for r in basins) == int((dg < 0).sum()), f"{what}: lowered_cells"
            assert sum(r["raised_cells"] for r in basins) == int((dg > 0).sum()), f"{what}: raised_cells"
        if clean:
            ds, dw = np.asarray(planes["dsolid"]).ravel(), np.asarray(planes["dwater"]).ravel()
            assert sum(r["deposited_q40"] - r["eroded_q40"] for r in basins) == sum(int(v) for v in ds), f"{what}: the dsolid plane does not sum to the net"
            assert sum(r["water_gained_q40"] - r["water_lost_q40"] for r in basins) == sum(int(v) for v in dw), f"{what}: the dwater plane"


def assert_all_zero(basins, soils, planes=None, what=""):
    """The budget of a map against an identical copy (flags aside: an unreliable term is unreliable in both)."""
    for r in basins:
        assert all(int(r[f]) == 0 for f in BASIN_FIELDS[2:] if f not in ("flags", "cut_max", "fill_max", "cut_cell", "fill_cell")), f"{what}: {r}"
        assert S.bits(r["cut_max"]) == 0 and S.bits(r["fill_max"]) == 0 and r["cut_cell"] == NONE and r["fill_cell"] == NONE, f"{what}: {r}"
    for q in soils:
        assert all(int(q[f]) == 0 for f in SOIL_FIELDS if f != "flags"), f"{what}: {q}"
    for p, v in (planes or {}).items():
        a = np.asarray(v)
        assert bool((a.view(np.uint64)[~np.isnan(a)] == 0).all()) if a.dtype == np.float64 else not a.any(), f"{what}: the {p} plane"


# ---- what a caller had before: the vectorised fold of two exported maps (tools/budget_bench.py times it) ----
def budget_np(base: Snapshot, now: Snapshot, labels: np.ndarray, ntypes: int):
    """The basins' counts and sums and the soils' gained / lost from two exports and the base's label plane, in numpy: the integers
    of budget() where no flag is raised."""
    def fold(s):
        cell = np.repeat(np.arange(s.ncells), s.count)
        q = np.floor(s.size * S.Q40).astype(np.uint64)
        hi, lo = (q >> np.uint64(32)).astype(np.float64), (q & np.uint64(0xFFFFFFFF)).astype(np.float64)

        def per_cell(m):                       # (the two 32-bit halves summed apart: exact in f64 weights)
            return (np.bincount(cell[m], hi[m], s.ncells).astype(np.uint64) << np.uint64(32)) + np.bincount(cell[m], lo[m], s.ncells).astype(np.uint64)

        v = np.stack([per_cell(s.type == t) for t in range(ntypes)])
        solid = per_cell(s.type != 0)
        end = np.cumsum(s.count.astype(np.int64))
        top = np.where(s.count > 0, end - 1, 0)
        ground = np.where(s.count > 0, np.where(s.type[top] == 0, s.floor[top], s.floor[top] + s.size[top]), 0.0)
        return v, solid, ground
    vb, sb, gb = fold(base)
    vn, sn, gn = fold(now)
    lab = np.asarray(labels).ravel()
    nb = int(lab.max()) + 1
    ds = sn.astype(np.int64) - sb.astype(np.int64)
    out = {"lowered_cells": np.bincount(lab, gn < gb, nb).astype(np.int64), "raised_cells": np.bincount(lab, gn > gb, nb).astype(np.int64),
           "eroded_q40": np.zeros(nb, np.int64), "deposited_q40": np.zeros(nb, np.int64)}
    np.add.at(out["eroded_q40"], lab, np.where(ds < 0, -ds, 0))
    np.add.at(out["deposited_q40"], lab, np.where(ds > 0, ds, 0))
    dv = vn.astype(np.int64) - vb.astype(np.int64)
    soils = [{"gained_q40": int(np.where(dv[t] > 0, dv[t], 0).sum()), "lost_q40": int(np.where(dv[t] < 0, -dv[t], 0).sum())} for t in range(ntypes)]
    return out, soils


# ---- the synthetic pairs: a base of drainage_ref and a "now" made of it by lowering, raising, burying and emptying columns ----
def columns_of(s: Snapshot) -> list:
    """One list per cell of (type, size, floor, sat), bottom -> top."""
    start, end = S._columns(s)
    ty, size, floor, sat = s.type.tolist(), s.size.tolist(), s.floor.tolist(), s.sat.tolist()
    return [[(ty[k], size[k], floor[k], sat[k]) for k in range(int(start[c]), int(end[c]))] for c in range(s.ncells)]


def snapshot_of(dimx: int, dimy: int, cols: list) -> Snapshot:
    count = np.array([len(c) for c in cols], np.uint32)
    flat = [sec for c in cols for sec in c]
    z = np.zeros(dimx * dimy, np.float32)
    arr = [np.array([sec[k] for sec in flat], dt) for k, dt in enumerate((np.uint32, np.float64, np.float64, np.float64))]
    return Snapshot(dimx, dimy, 80, 65, 0, 0, count, *arr, z, z.copy(), z.copy())


NEW_TYPES = (1, 2, 3, 4, 5, 31, 63, 64, 100)   # 5: the first type beyond the kernel's registers; 63: the last of a table; 64, 100: beyond every table
TIE = 8.0                                       # deeper than every other cut of the pairs


def edited(base: Snapshot):
    """(now, notes): `now` is base with the column of cell c changed by rule c % 12; notes names the cells of the special cases."""
    cols = columns_of(base)
    n = len(cols)
    notes = {}

    def top_h(col):
        return col[-1][2] + col[-1][1] if col else 0.0

    plain = [c for c, col in enumerate(cols) if len(col) == 1 and col[0][0] != 0 and c % 12 in (0, 10, 11)]   # dry, one section, no rule
    for c, col in enumerate(cols):
        k = c % 12
        if not col:
            if c != n - 1:                                   # empty -> filled (the last cell stays empty in both)
                cols[c] = [(1, 0.5, 0.0, 0.0), (2, 0.25, 0.5, 0.5)]
                notes.setdefault("filled", c)
            continue
        t, sz, fl, st = col[-1]
        if k == 1:                                           # lowered: a part of the top section goes
            col[-1] = (t, sz - 2.0 ** -7 if sz >= 2.0 ** -7 else sz * 0.5, fl, st)
        elif k == 2:                                         # raised: a new section, the types in turn
            col.append((NEW_TYPES[(c // 12) % len(NEW_TYPES)], 0.125 + (c % 5) * 2.0 ** -6, top_h(col), 0.25 * (c % 3)))
        elif k == 3:                                         # the top section goes: another top, or none
            col.pop()
            if not col:
                notes.setdefault("emptied", c)
        elif k == 4:                                         # buried under water
            col.append((0, 2.0 ** -5, top_h(col), 1.0))
        elif k == 5 and c % 24 == 5:                         # filled -> empty
            cols[c] = []
            notes.setdefault("emptied", c)
        elif k == 6:                                         # a section under the column: S changes, the ground does not
            col.insert(0, (5, 0.375, col[0][2] - 0.375, 0.5))
        elif k == 7:                                         # the same ground under another name
            col[-1] = (t + 1, sz, fl, st)
        elif k == 8:                                         # wetter: only H changes
            col[-1] = (t, sz, fl, 0.75)
        elif k == 9:                                         # two sections in place of the top one, the same ground where the halves add up
            col[-1] = (t, sz * 0.5, fl, st)
            col.append((63, sz * 0.5, fl + sz * 0.5, 0.5))
    # the special cases, on cells the rules above left alone or not: each replaces its column
    if len(plain) >= 5:
        a, b, big, nan, neg = plain[0], plain[len(plain) // 2], plain[1], plain[2], plain[-1]
        for c in (a, b):                                     # two cells tie for the deepest cut: the floor goes down by TIE, the sizes stay
            t, sz, fl, st = cols[c][-1]
            cols[c] = [(t, sz, fl - TIE, st)]
        t, sz, fl, st = cols[big][-1]
        cols[big] = [(t, sz, fl, st), (3, 16777216.0, fl + sz, 0.0)]      # a size of 2^24: it contributes 0 and raises the flag
        t, sz, fl, st = cols[nan][-1]
        cols[nan] = [(t, sz, float("nan"), st)]               # a NaN floor: neither lowered nor raised
        t, sz, fl, st = cols[neg][-1]
        cols[neg] = [(t, sz, fl, st), (2, 0.5, fl + sz, float("inf"))]    # size * sat is not finite: the held term alone is unreliable
        notes.update(tie=(a, b), big=big, nan=nan, held=neg)
    return snapshot_of(base.dimx, base.dimy, cols), notes


PAIR_INPUTS = ("cone", "ties", "random_bernoulli20", "empty")
PAIR_DIMS = ((9, 7), (33, 47), (65, 63), (1, 70), (70, 1))
_pairs = {}


def pair(name: str, dims: tuple):
    """(base, now, notes, the base's drainage) of a synthetic pair, made once and shared."""
    k = (name, tuple(dims))
    if k not in _pairs:
        base, drain = D.case(name, dims)
        now, notes = edited(base)
        _pairs[k] = (base, now, notes, drain)
    return _pairs[k]


_wants = {}


def want(name: str, dims: tuple, ntypes: int):
    """budget() of a synthetic pair, computed once per ntypes."""
    k = (name, tuple(dims), ntypes)
    if k not in _wants:
        base, now, _, drain = pair(name, dims)
        _wants[k] = budget(base, now, ntypes, drain)
    return _wants[k]
