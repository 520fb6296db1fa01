"""numpy statements of what smx_ensemble_figures / smx_ensemble_plane_stats return (include/soilmx.h), for the tests on both sides."""
from __future__ import annotations

import numpy as np

from soilmachine_amd.snapshot import Snapshot


def seq_sum(a) -> float:
    """Sequential f64 accumulation in index order (numpy's own .sum() is pairwise: other bits)."""
    acc = 0.0
    for v in a:
        acc += float(v)
    return acc


def tops(s: Snapshot):
    """(non-empty mask, index of each non-empty column's top section, whether that top is water) -- tools/p2_reference.py:149-151."""
    end = np.cumsum(s.count.astype(np.int64)); nz = s.count > 0
    top = end[nz] - 1
    air = s.type[top] == 0
    return nz, top, air


def figures_ref(s: Snapshot) -> dict:
    """The fields of smx_member_figures a snapshot defines (rand_calls / live_sections are the context's own words)."""
    nz, top, air = tops(s)
    h = s.heights()
    d = s.digest()
    return {"sumh": d["sumh"], "nsec": d["nsec"], "typehash": d["typehash"],
            "wet_cells": int(air.sum()),                                   # "standing" of tools/p2_reference.py:153
            "water_volume": seq_sum(s.size[top][air]),                      # its water_volume, folded sequentially in cell order
            "hmin": float(h.min()), "hmax": float(h.max()), "empty_cells": int((~nz).sum())}


def water_plane(s: Snapshot) -> np.ndarray:
    """SMX_PLANE_WATER of one member: the top section's size where it is water, else 0 (cell order)."""
    nz, top, air = tops(s)
    w = np.zeros(s.ncells)
    w[nz] = np.where(air, s.size[top], 0.0)
    return w


def stats_ref(vs, var: bool = True) -> dict:
    """The member loop of smx_ensemble_plane_stats over the planes `vs` (f64, or f32 to be widened), in that order."""
    vs = [np.asarray(v).astype(np.float64).ravel() for v in vs]
    n = len(vs)
    acc = np.zeros_like(vs[0])
    vmin, vmax = vs[0].copy(), vs[0].copy()
    nonzero = np.zeros(vs[0].shape, np.uint32)
    for i, v in enumerate(vs):
        acc += v
        if i:
            vmin = np.where(v < vmin, v, vmin)
            vmax = np.where(v > vmax, v, vmax)
        nonzero += (v != 0.0).astype(np.uint32)
    out = {"mean": acc / float(n), "vmin": vmin, "vmax": vmax, "nonzero": nonzero}
    if var:
        a2 = np.zeros_like(vs[0])
        for v in vs:
            d = v - out["mean"]
            a2 += d * d
        out["var"] = a2 / float(n)
    return out


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(np.array_equal(a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")))
    return bool(np.array_equal(a, b))


def f64_bits(x: float) -> int:
    return int(np.array([x], np.float64).view(np.uint64)[0])
