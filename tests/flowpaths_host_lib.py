"""ctypes wrapper of tests/flowpaths_host (soil_paths.h compiled for the host -- TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flowpaths_host")
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libflowpaths_host.so")
SRC = [os.path.join(HERE, "flowpaths_host.cpp"), os.path.join(os.path.dirname(HERE), "drainage_host", "drainage_host.cpp")] + \
      [os.path.join(ROOT, "soilmachine_amd", "csrc", f) for f in ("soil_core.h", "soil_lakes.h", "soil_drain.h", "soil_streams.h", "soil_hills.h", "soil_paths.h")]
PLANES = ("terminal", "straight", "diagonal", "drop", "upstream", "source", "stem")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in SRC):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", LIB, SRC[0]])
        L = C.CDLL(LIB)
        vp = C.c_void_p
        L.dh_create.restype = vp
        L.dh_create.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp]
        L.dh_destroy.argtypes = [vp]; L.dh_destroy.restype = None
        L.dh_variant.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3
        L.fh_flowpaths.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32, vp, vp] + [vp] * 7 + [vp, C.c_uint32, vp, C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


def variants() -> dict:
    """variant -> (tile columns, tile rows, slots of the fold's table): the shapes of the drainage host build"""
    L = lib()
    out = {}
    for v in range(L.dh_variants()):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        assert L.dh_variant(v, C.byref(a), C.byref(b), C.byref(c)) == 0
        out[v] = (a.value, b.value, c.value)
    return out


class HostMap:
    """The top records of one snapshot's columns on the host."""

    def __init__(self, s: Snapshot):
        self.L = lib()
        self.dimx, self.dimy = int(s.dimx), int(s.dimy)
        arr = [np.ascontiguousarray(a, dt) for a, dt in ((s.count, np.uint32), (s.type, np.uint32), (s.size, np.float64), (s.floor, np.float64))]
        self.h = self.L.dh_create(self.dimx, self.dimy, *[capi.ptr(a) for a in arr])

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dh_destroy(self.h); self.h = None


def flowpaths_many(maps, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=PLANES, profile_cap: int | None = None):
    """The kernels' bodies over `maps` in one go (the ensemble path) -> one (records, planes, profile, nbasins, nprofile, rounds) per
    map; cap None: two calls, a count and the fetch, as the Python binding does. order: bit 0 the workgroups, bit 1 the lanes, last to
    first; bits 2 and 3 flip those two for the up-walk alone. profile_cap (one map only): None = no profile."""
    L = lib()
    n = len(maps)
    hs = (C.c_void_p * n)(*[m.h for m in maps])
    ns, nps = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rounds = C.c_uint32()
    if cap is None:
        assert L.fh_flowpaths(hs, n, variant, lanes, order, 0, None, capi.ptr(ns), *[None] * 7, None, 0, capi.ptr(nps), None) == 0
        cap = int(ns.max()) if n else 0
    out = (capi.Flowpath * max(1, n * cap))()
    words = sum(m.dimx * m.dimy for m in maps)
    pl = {k: np.zeros(words, np.float64 if k == "drop" else np.uint32) for k in planes}
    prof = np.full(max(1, profile_cap or 0), 0xFFFFFFFF, np.uint32)
    assert L.fh_flowpaths(hs, n, variant, lanes, order, cap, out, capi.ptr(ns), *[capi.ptr(pl.get(k)) for k in PLANES],
                          capi.ptr(prof) if profile_cap else None, profile_cap or 0, capi.ptr(nps), C.byref(rounds)) == 0
    res, at = [], 0
    for i, m in enumerate(maps):
        k = min(cap, int(ns[i]))
        cells = m.dimx * m.dimy
        res.append(([out[i * cap + r].as_dict() for r in range(k)], {p: v[at:at + cells].reshape(m.dimx, m.dimy).copy() for p, v in pl.items()},
                    prof[:min(profile_cap, int(nps[i]))].copy() if profile_cap is not None else None, int(ns[i]), int(nps[i]), int(rounds.value)))
        at += cells
    return res


def flowpaths(s, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=PLANES, profile_cap: int | None = -1):
    """(records, planes, profile, nbasins, nprofile, rounds) of one snapshot; profile_cap -1: room for every cell."""
    m = HostMap(s)
    return flowpaths_many([m], variant, lanes, order, cap, planes, m.dimx * m.dimy if profile_cap == -1 else profile_cap)[0]
