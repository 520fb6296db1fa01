"""Dispersed flow restated in plain Python loops (include/soilmx.h, "dispersed flow") -- TEST INFRASTRUCTURE ONLY.

On top of drainage_ref: heights, wet cells, receivers and basin ranks are the drainage's. A dry cell with a lower neighbour (plain
f64 `<`) is a giver; it hands share(n) = (A * f(n)) >> 24 to every lower neighbour and the remainder to its receiver, with
f(n) = int((w(n) / W) * 2^24), w(n) = 1.0 * s * s ... (`exponent` factors) and s = (h(c) - h(n)) * k. Python floats are IEEE doubles
and Python multiplies and adds them one operation at a time, so the fractions are the library's bit for bit; the areas are ints.
"""
from __future__ import annotations

import math

import numpy as np

import drainage_ref as D
import lakes_ref as L
from soilmachine_amd.snapshot import Snapshot

ONE = 1 << 24
NONE = 0xFFFFFFFF
DIAG = float.fromhex("0x1.6a09e667f3bcdp-1")          # 0x3FE6A09E667F3BCD
FIELDS = ("first_cell", "cells", "flags", "peak_cell", "inflow_q24", "leak_in_q24", "leak_out_q24", "peak_q24", "givers", "split_cells")
PLANES = ("area", "donors", "receivers")


def fractions(hc: float, lower: list, exponent: int) -> list:
    """lower: [(h(n), diagonal)] in ascending cell index -> [f(n)]"""
    ws, W = [], 0.0
    for hn, diag in lower:
        s = (hc - hn) * (DIAG if diag else 1.0)
        w = 1.0
        for _ in range(exponent):
            w = w * s
        ws.append(w)
        W = W + w
    if not (W > 0.0 and math.isfinite(W)):
        return [0] * len(ws)
    return [int((w / W) * 16777216.0) for w in ws]


def dispersal(s: Snapshot, exponent: int = 1, drainage=None):
    """(records, planes): one dict per basin of drainage_ref.drainage(s) in rank order; the (dimx, dimy) planes `area` (uint64),
    `donors` and `receivers` (uint32). drainage: that call's result, where the caller has it."""
    assert 0 <= exponent <= 16
    dimx, dimy = int(s.dimx), int(s.dimy)
    n = dimx * dimy
    wet, h = D.heights(s)
    hl = [float(v) for v in h]
    drecs, dplanes = (drainage or D.drainage(s))[:2]
    recv = [int(v) for v in dplanes["receivers"].reshape(n)]
    label = [int(v) for v in dplanes["labels"].reshape(n)]
    lower = [[] for _ in range(n)]                   # per giver: (n, diagonal) in ascending cell index
    donors = [0] * n
    for c in range(n):
        if wet[c]:
            continue
        x, y = divmod(c, dimy)
        for dx, dy in L.NB8:                         # ascending cell index
            u, v = x + dx, y + dy
            if 0 <= u < dimx and 0 <= v < dimy and hl[u * dimy + v] < hl[c]:
                lower[c].append((u * dimy + v, dx != 0 and dy != 0))
                donors[u * dimy + v] += 1
    area = [ONE] * n
    leak_in = [0] * len(drecs)
    leak_out = [0] * len(drecs)
    givers = [c for c in range(n) if lower[c]]
    # a receiver is strictly lower than its giver: in descending h every giver is complete when its turn comes (a NaN is no giver)
    givers.sort(key=lambda c: hl[c], reverse=True)
    for c in givers:
        assert recv[c] in [m for m, _ in lower[c]]
        fs = fractions(hl[c], [(hl[m], dg) for m, dg in lower[c]], exponent)
        assert sum(fs) <= ONE
        shares = [(area[c] * f) >> 24 for f in fs]
        rem = area[c] - sum(shares)
        assert rem >= 0
        for (m, _), sh in zip(lower[c], shares):
            amount = sh + (rem if m == recv[c] else 0)
            area[m] += amount
            if label[m] != label[c]:
                leak_out[label[c]] += amount
                leak_in[label[m]] += amount
    recs = []
    members = [[] for _ in drecs]
    for c in range(n):
        members[label[c]].append(c)
    for k, (b, cells) in enumerate(zip(drecs, members)):
        dry = [c for c in cells if not wet[c]]
        peak = max((area[c] for c in dry), default=0)
        recs.append({"first_cell": b["first_cell"], "cells": b["cells"], "flags": b["flags"],
                     "peak_cell": min((c for c in dry if area[c] == peak), default=NONE),
                     "inflow_q24": sum(area[c] for c in cells if recv[c] == NONE), "leak_in_q24": leak_in[k], "leak_out_q24": leak_out[k], "peak_q24": peak,
                     "givers": sum(1 for c in cells if lower[c]), "split_cells": sum(1 for c in cells if len(lower[c]) >= 2)})
    planes = {"area": np.array(area, np.uint64).reshape(dimx, dimy), "donors": np.array(donors, np.uint32).reshape(dimx, dimy),
              "receivers": np.array([len(v) for v in lower], np.uint32).reshape(dimx, dimy)}
    return recs, planes


def same(a: dict, b: dict) -> list:
    return [f"{f}: {a[f]} vs {b[f]}" for f in FIELDS if int(a[f]) != int(b[f])]


def assert_same_dispersal(got, want, what="", count=None):
    """got / want = (records, planes); planes: a dict that may lack a plane (or None). `count`: the number of basins the caller
    was told, where it has one."""
    gr, gp, wr, wp = got[0], got[1] or {}, want[0], want[1] or {}
    if count is not None:
        assert count == len(wr), f"{what}: {count} basins counted, expected {len(wr)}"
    assert len(gr) == len(wr), f"{what}: {len(gr)} basins, expected {len(wr)}"
    for k, (a, b) in enumerate(zip(gr, wr)):
        bad = same(a, b)
        assert not bad, f"{what}: basin {k}: " + "; ".join(bad)
    for p in PLANES:
        if gp.get(p) is not None and wp.get(p) is not None:
            g, w = np.asarray(gp[p], wp[p].dtype).reshape(wp[p].shape), wp[p]
            assert np.array_equal(g, w), f"{what}: the {p} planes differ at {int((g != w).sum())} cells, the first at cell {int(np.flatnonzero(g != w)[0])}"


def assert_invariants(s: Snapshot, recs, planes=None, what=""):
    """What holds for every map: the three conservation laws, exactly; with the planes, A(c) >= ONE, the areas of the terminal cells
    sum to the map, and the donors and receivers planes agree with the heights."""
    dimx, dimy = int(s.dimx), int(s.dimy)
    n = dimx * dimy
    for r in recs:
        assert r["inflow_q24"] == r["cells"] * ONE + r["leak_in_q24"] - r["leak_out_q24"], f"{what}: the balance of basin {r['first_cell']}"
    assert sum(r["inflow_q24"] for r in recs) == n * ONE, f"{what}: the inflows do not sum to the map"
    assert sum(r["leak_in_q24"] for r in recs) == sum(r["leak_out_q24"] for r in recs), f"{what}: leak_in and leak_out differ"
    if not planes:
        return
    wet, h = D.heights(s)
    hl = [float(v) for v in h]
    if planes.get("area") is not None:
        area = [int(v) for v in np.asarray(planes["area"]).reshape(n)]
        assert min(area) >= ONE, f"{what}: an area below ONE"
    want_d, want_r = [0] * n, [0] * n
    for c in range(n):
        x, y = divmod(c, dimy)
        for dx, dy in L.NB8:
            u, v = x + dx, y + dy
            if 0 <= u < dimx and 0 <= v < dimy:
                m = u * dimy + v
                if not wet[c] and hl[m] < hl[c]:
                    want_r[c] += 1
                if not wet[m] and hl[c] < hl[m]:
                    want_d[c] += 1
    if planes.get("donors") is not None:
        assert [int(v) for v in np.asarray(planes["donors"]).reshape(n)] == want_d, f"{what}: the donors plane disagrees with the heights"
    if planes.get("receivers") is not None:
        assert [int(v) for v in np.asarray(planes["receivers"]).reshape(n)] == want_r, f"{what}: the receivers plane disagrees with the heights"
    if planes.get("area") is not None and planes.get("receivers") is not None:
        assert sum(a for a, r, w in zip(area, want_r, wet) if w or r == 0) == n * ONE, f"{what}: the areas of the sinks and the wet cells do not sum to the map"


# ---- the hand-built 16 x 16 map ----
def hand_map() -> Snapshot:
    """A floor of height 100 (a floor cell with no feature beside it is a sink, a basin of its own) with four features, far enough
    apart not to meet:
      a cone corner  cell (0, 0) = 103: its three neighbours are floor sinks, it splits three ways.
      a divide       cell (2, 8) = 105 between the pits (2, 7) = 90 and (2, 9) = 95: all eight neighbours are lower, and so does the
                     floor cell (1, 8) above it: both leak into two basins.
      a lake         wet cells (8, 3) and (8, 4) at 99 + 2^-11, entered from (7, 3) = 104 on one side and (9, 4) = 106 on the other
                     (and by the floor around it).
      a lake without dry land: wet cells (12..13, 12..13) at 150 + 2^-11, above the floor around them, which stays sinks.
    The numbers are written out in tests/test_dispersal_host.py (HAND)."""
    dx = dy = 16
    h = np.full((dx, dy), 100.0)
    wet = np.zeros((dx, dy), bool)
    h[0, 0] = 103.0
    h[2, 7], h[2, 8], h[2, 9] = 90.0, 105.0, 95.0
    wet[8, 3] = wet[8, 4] = True
    h[8, 3] = h[8, 4] = 99.0
    h[7, 3], h[9, 4] = 104.0, 106.0
    wet[12:14, 12:14] = True
    h[12:14, 12:14] = 150.0
    return L.make_snapshot(wet, np.full((dx, dy), 2.0 ** -11), h.reshape(dx, dy), ())


EXPONENTS = (0, 1, 4)
_cases = {}


def case(name: str, dims: tuple, exponent: int):
    """(snapshot, drainage, dispersal) of an input, computed once and shared by the tests that need it."""
    k = (name, tuple(dims), exponent)
    if k not in _cases:
        s, drain = (hand_map(), None) if name == "hand" else D.case(name, dims)
        if drain is None:
            drain = _cases[(name, tuple(dims), EXPONENTS[0])][1] if (name, tuple(dims), EXPONENTS[0]) in _cases else D.drainage(s)
        _cases[k] = (s, drain, dispersal(s, exponent, drain))
    return _cases[k]


def hand_case(exponent: int):
    return case("hand", (16, 16), exponent)
