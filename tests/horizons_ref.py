"""The horizons restated in plain loops (include/soilmx.h, "horizons") -- TEST INFRASTRUCTURE ONLY.

numpy over the cells, a Python loop over the steps k and the directions d: EVERY step of every ray is looked at, no tile is skipped.
h(c) is drainage_ref.heights (floor + size of the top record in one f64 addition, 0.0 for an empty column). The ray of c = (x, y) in
direction d is c_k = (x + k ux, y + k uy), k = 1, 2, ... while it lies in the map and k <= reach (0: no limit);
s_k = (h(c_k) - h(c)) / (float(k) * len(d)); K is the smallest k with the largest s_k > +0.0 (plain >), S that s_k; 0 and +0.0 where
there is none.
"""
from __future__ import annotations

import struct

import numpy as np

import drainage_ref as D
import lakes_ref as L
from soilmachine_amd.snapshot import Snapshot

NONE = 0xFFFFFFFF
DIRS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1), (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2), (1, -1), (2, -1))
SQRT2 = struct.unpack("<d", struct.pack("<Q", 0x3FF6A09E667F3BCD))[0]
SQRT5 = struct.unpack("<d", struct.pack("<Q", 0x4001E3779B97F4A8))[0]
LEN = tuple(SQRT5 if d & 1 else SQRT2 if d & 2 else 1.0 for d in range(16))
FIELDS = ("direction", "ux", "uy", "bounded", "step_max", "step_max_cell", "step_sum", "slope_max")
PLANES = ("slope", "step", "sky", "open", "lit")
REACHES = (0, 1, 5)


def selected(mask: int) -> list:
    return [d for d in range(16) if mask >> d & 1]


def surface(s: Snapshot) -> np.ndarray:
    """h as a (dimx, dimy) array."""
    return D.heights(s)[1].reshape(int(s.dimx), int(s.dimy))


def rays(h: np.ndarray, d: int, reach: int = 0):
    """(S, K) of direction d: every step of every ray, the winners kept per cell."""
    dx, dy = h.shape
    ux, uy = DIRS[d]
    best = np.zeros((dx, dy))
    bk = np.zeros((dx, dy), np.uint32)
    k = 1
    with np.errstate(all="ignore"):
        while not (reach and k > reach):
            x0, x1, y0, y1 = max(0, -k * ux), min(dx, dx - k * ux), max(0, -k * uy), min(dy, dy - k * uy)
            if x0 >= x1 or y0 >= y1:
                break
            sk = (h[x0 + k * ux:x1 + k * ux, y0 + k * uy:y1 + k * uy] - h[x0:x1, y0:y1]) / (float(k) * LEN[d])
            b, kk = best[x0:x1, y0:y1], bk[x0:x1, y0:y1]
            win = sk > b
            b[win] = sk[win]
            kk[win] = k
            k += 1
    return best, bk


def horizons(s: Snapshot, mask: int = 0xFFFF, reach: int = 0, suns=()):
    """(records, planes, lit_cells): one dict per selected direction; planes = {"slope": (nd, dimx, dimy) f64, "step": the same u32,
    "sky": (dimx, dimy) f64, "open", "lit": u32}; lit_cells: a count per sun. suns: (d, tangent) pairs."""
    h = surface(s)
    ds = selected(mask)
    sk = [rays(h, d, reach) for d in ds]
    S = np.array([a for a, _ in sk]).reshape(len(ds), *h.shape)
    K = np.array([b for _, b in sk], np.uint32).reshape(len(ds), *h.shape)
    return (fold_records(ds, S, K),) + derived(ds, S, K, suns)


def fold_records(ds, S, K) -> list:
    recs = []
    for j, d in enumerate(ds):
        k, sl = K[j].reshape(-1), S[j].reshape(-1)
        bounded = int((k != 0).sum())
        recs.append({"direction": d, "ux": DIRS[d][0], "uy": DIRS[d][1], "bounded": bounded, "step_max": int(k.max()) if k.size else 0,
                     "step_max_cell": int(np.flatnonzero(k == k.max())[0]) if bounded else NONE, "step_sum": int(k.astype(np.uint64).sum()),
                     "slope_max": max((float(v) for v in sl[k != 0]), key=L.key) if bounded else 0.0})
    return recs


def derived(ds, S, K, suns=()):
    """(planes, lit_cells) from the slopes and steps of the selected directions."""
    acc = np.zeros(S.shape[1:])
    op = np.zeros(S.shape[1:], np.uint32)
    with np.errstate(all="ignore"):
        for j, d in enumerate(ds):
            acc = acc + 1.0 / (1.0 + S[j] * S[j])
            op |= np.where(K[j] == 0, np.uint32(1 << d), np.uint32(0))
        sky = acc / float(len(ds))
    lit = np.zeros(S.shape[1:], np.uint32)
    counts = []
    for d, tangent in suns:
        on = ~(S[ds.index(d)] > float(tangent))
        lit += on.astype(np.uint32)
        counts.append(int(on.sum()))
    return {"slope": S, "step": K, "sky": sky, "open": op, "lit": lit}, counts


def attach(recs, suns, counts) -> list:
    """The records with lit_cells as the Python binding hands them out: per record the counts of the suns of its direction."""
    out = [dict(r) for r in recs]
    for r in out:
        r["lit_cells"] = [int(counts[i]) for i, (d, _) in enumerate(suns) if d == r["direction"]]
    return out


def same(a: dict, b: dict) -> list:
    """Field-by-field comparison of two records, floats by their bits; the list of differing fields."""
    bad = []
    for f in FIELDS:
        u, v = a[f], b[f]
        if f == "slope_max":
            if L.bits(u) != L.bits(v):
                bad.append(f"{f}: {u!r} vs {v!r}")
        elif int(u) != int(v):
            bad.append(f"{f}: {u} vs {v}")
    if "lit_cells" in a and "lit_cells" in b and list(a["lit_cells"]) != list(b["lit_cells"]):
        bad.append(f"lit_cells: {a['lit_cells']} vs {b['lit_cells']}")
    return bad


def assert_same_horizons(got, want, what=""):
    """got / want = (records, planes or None[, lit_cells or None]); a plane either side lacks is not compared. Doubles by their bits."""
    gr, gp, wr, wp = got[0], got[1] or {}, want[0], want[1] or {}
    assert len(gr) == len(wr), f"{what}: {len(gr)} records, expected {len(wr)}"
    for k, (a, b) in enumerate(zip(gr, wr)):
        bad = same(a, b)
        assert not bad, f"{what}: record {k} (direction {b['direction']}): " + "; ".join(bad)
    for p in PLANES:
        if gp.get(p) is not None and wp.get(p) is not None:
            w = np.ascontiguousarray(wp[p])
            g = np.ascontiguousarray(np.asarray(gp[p], w.dtype).reshape(w.shape))
            u = np.uint64 if w.dtype == np.float64 else np.uint32
            diff = g.view(u) != w.view(u)
            if diff.any():
                at = tuple(int(v) for v in np.argwhere(diff)[0])
                raise AssertionError(f"{what}: the {p} planes differ at {int(diff.sum())} places, the first at {at}: {g[at]!r} vs {w[at]!r}")
    if len(got) > 2 and len(want) > 2 and got[2] is not None and want[2] is not None:
        assert [int(v) for v in got[2]] == [int(v) for v in want[2]], f"{what}: lit_cells {list(got[2])} vs {list(want[2])}"


def transposed(s: Snapshot) -> Snapshot:
    """The map with x and y exchanged (the top records only: one section a column, wet cells as a second one)."""
    dx, dy = int(s.dimx), int(s.dimy)
    wet, size, floor = L.tops(s)
    empty = np.flatnonzero(np.asarray(s.count).reshape(dx, dy).T.reshape(-1) == 0)
    t = lambda a: np.asarray(a).reshape(dx, dy).T
    return L.make_snapshot(t(wet), t(size), np.where(t(wet), t(floor), t(floor + size)), [int(c) for c in empty])


def assert_invariants(s: Snapshot, mask: int, reach: int, suns, recs, planes, lit_cells, what=""):
    """What holds for every map, checked on (recs, planes, lit_cells) as somebody computed them for (mask, reach, suns) with ALL
    planes: S > 0 exactly where K > 0, and h(c_K) > h(c); a reach gives the unlimited result wherever the unlimited K <= reach and is
    nowhere larger; sky == 1.0 exactly where open holds every selected bit; a sub-mask gives the same bits for its directions; the
    records are folds of the planes and lit_cells counts of lit's contributions; the transposed map gives the transposed planes under
    (ux, uy) -> (uy, ux)."""
    h = surface(s)
    dx, dy = h.shape
    ds = selected(mask)
    S, K = np.asarray(planes["slope"]).reshape(len(ds), dx, dy), np.asarray(planes["step"]).reshape(len(ds), dx, dy)
    xs, ys = np.indices((dx, dy))
    for j, d in enumerate(ds):
        assert np.array_equal(S[j] > 0, K[j] > 0), f"{what}: direction {d}: S > 0 is not where K > 0"
        assert (S[j].view(np.uint64)[K[j] == 0] == 0).all(), f"{what}: direction {d}: S is not +0.0 where K == 0"
        px, py = xs + K[j].astype(np.int64) * DIRS[d][0], ys + K[j].astype(np.int64) * DIRS[d][1]
        assert ((px >= 0) & (px < dx) & (py >= 0) & (py < dy)).all(), f"{what}: direction {d}: a horizon outside the map"
        on = K[j] > 0
        assert (h[px[on], py[on]] > h[on]).all(), f"{what}: direction {d}: a horizon cell that is not above its cell"
        if reach:
            assert (K[j] <= reach).all(), f"{what}: direction {d}: a step beyond the reach"
            fs, fk = rays(h, d, 0)
            near = fk <= reach
            assert np.array_equal(K[j][near], fk[near]) and np.array_equal(S[j].view(np.uint64)[near], fs.view(np.uint64)[near]), f"{what}: direction {d}: the reach changed a near horizon"
            assert not (S[j] > fs).any(), f"{what}: direction {d}: a horizon within the reach above the unlimited one"
    sky, op = np.asarray(planes["sky"]).reshape(dx, dy), np.asarray(planes["open"]).reshape(dx, dy)
    assert np.array_equal(sky == 1.0, op == mask), f"{what}: sky == 1.0 is not where every selected direction is open"
    assert ((op & ~np.uint32(mask)) == 0).all(), f"{what}: an open bit outside the mask"
    if len(ds) > 1:                                            # a sub-mask: every other selected direction
        sub = ds[::2]
        want = horizons(s, sum(1 << d for d in sub), reach)
        for i, d in enumerate(sub):
            j = ds.index(d)
            assert np.array_equal(want[1]["step"][i], K[j]) and np.array_equal(want[1]["slope"][i].view(np.uint64), S[j].view(np.uint64)), f"{what}: direction {d} differs under a sub-mask"
    folded = fold_records(ds, S, K)
    for a, b in zip(recs, folded):
        assert not same(a, b), f"{what}: record of direction {b['direction']} is not the fold of its planes: " + "; ".join(same(a, b))
    pl, counts = derived(ds, S, K, suns)
    assert_same_horizons((folded, {k: planes[k] for k in ("sky", "open", "lit") if planes.get(k) is not None}, lit_cells), (folded, pl, counts), f"{what}: derived from slope and step")
    ts = transposed(s)
    swap = {d: DIRS.index((DIRS[d][1], DIRS[d][0])) for d in ds}
    th = surface(ts)
    assert np.array_equal(th, h.T, equal_nan=True)           # (a -0.0 may have become +0.0: no difference of heights is > 0 for it)
    for j, d in enumerate(ds):
        a, b = rays(th, swap[d], reach)
        assert np.array_equal(b, K[j].T) and np.array_equal(a.view(np.uint64), np.ascontiguousarray(S[j].T).view(np.uint64)), f"{what}: direction {d}: the transposed map"


# ---- the inputs of their own ----
def _snap(dx, dy, h, wet=None, depth=None, empty=()):
    return L.make_snapshot(np.zeros((dx, dy), bool) if wet is None else wet, depth, np.asarray(h, np.float64).reshape(dx, dy), empty)


def i_integer_ties(dx, dy):
    """Random integers 0..5: most horizons are shared by several steps."""
    return _snap(dx, dy, np.random.default_rng(31).integers(0, 6, (dx, dy)).astype(np.float64))


def i_nan_inf(dx, dy):
    """Random floats sprinkled with NaN, +inf and -inf."""
    rng = np.random.default_rng(32)
    h = rng.random((dx, dy)) * 8.0
    r = rng.random((dx, dy))
    h[r < 0.03] = np.nan
    h[(r >= 0.03) & (r < 0.05)] = np.inf
    h[(r >= 0.05) & (r < 0.07)] = -np.inf
    return _snap(dx, dy, h)


def i_spike(dx, dy):
    """Flat ground with one tall cell: every ray that meets it has it as its horizon, however far."""
    h = np.full((dx, dy), 1.0)
    h[(2 * dx) // 3, dy // 3] = 1000.0
    return _snap(dx, dy, h)


def i_ramp(dx, dy):
    """h = x: along +x every s_k is k / k == 1.0 exactly, so the horizon ties at every k and K == 1."""
    return _snap(dx, dy, np.repeat(np.arange(dx, dtype=np.float64), dy))


def i_wall(dx, dy):
    """Low ground, then a step up across the middle of whichever axis is longer."""
    h = np.zeros((dx, dy))
    if dx >= dy:
        h[dx // 2:, :] = 5.0
    else:
        h[:, dy // 2:] = 5.0
    return _snap(dx, dy, h)


def i_bowl_lake(dx, dy):
    """A bowl with a lake in its middle: the lake's surface, not its bed, is what the rays see."""
    x, y = np.indices((dx, dy))
    r2 = (x - dx // 2) ** 2 + (y - dy // 2) ** 2
    bed = r2 * 2.0 ** -6
    level = float(bed.max()) * 0.25
    wet = bed < level
    return _snap(dx, dy, bed, wet, np.where(wet, level - bed, 0.25))


def i_empty(dx, dy):
    return D.i_empty(dx, dy)


def i_extremes(dx, dy):
    """Integer ties scaled into the subnormal range on one half of the map and to the brink of overflow on the other: slopes that
    underflow, products of a slope and a distance that overflow -- where a comparison must not be decided without the division."""
    h = np.random.default_rng(33).integers(0, 6, (dx, dy)).astype(np.float64)
    big = (np.arange(dx)[:, None] if dx >= dy else np.arange(dy)[None, :]) >= max(dx, dy) // 2
    return _snap(dx, dy, np.where(big, h * 2.0 ** 1021, h * 2.0 ** -1071))


INPUTS = {"integer_ties": i_integer_ties, "nan_inf": i_nan_inf, "spike": i_spike, "ramp": i_ramp, "wall": i_wall, "bowl_lake": i_bowl_lake, "empty": i_empty,
          "extremes": i_extremes}
SUN_TANGENTS = (0.0, 0.5, 1.0e6)       # on the horizon, a slope that occurs on the integer maps (1 / 2), practically overhead

_cases = {}


def snapshot_of(name: str, dims: tuple) -> Snapshot:
    return (INPUTS[name] if name in INPUTS else D.INPUTS[name])(*dims)


def suns_for(mask: int) -> list:
    """Three suns for the first, the middle and the last selected direction, one of each tangent."""
    ds = selected(mask)
    return [(ds[0], SUN_TANGENTS[0]), (ds[len(ds) // 2], SUN_TANGENTS[1]), (ds[-1], SUN_TANGENTS[2])]


def case(name: str, dims: tuple, mask: int = 0xFFFF, reach: int = 0):
    """(snapshot, suns, (records with lit_cells, planes, lit_cells)) of an input, computed once and shared by the tests that need it."""
    k = (name, tuple(dims), mask, reach)
    if k not in _cases:
        s = snapshot_of(name, dims)
        suns = suns_for(mask)
        recs, planes, counts = horizons(s, mask, reach, suns)
        _cases[k] = (s, suns, (attach(recs, suns, counts), planes, counts))
    return _cases[k]
