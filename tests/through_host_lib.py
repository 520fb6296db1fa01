"""ctypes wrapper of tests/through_host (soil_through.h compiled for the host -- TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import drainage_host_lib as DH
from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "through_host")
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libthrough_host.so")
SRC = [os.path.join(HERE, "through_host.cpp"), os.path.join(DH.HERE, "drainage_host.cpp")] + \
      [os.path.join(ROOT, "soilmachine_amd", "csrc", f) for f in ("soil_core.h", "soil_lakes.h", "soil_drain.h", "soil_spill.h", "soil_through.h")]
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
        L.th_variant.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 4
        L.th_batch.restype = C.c_uint32
        L.th_through.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp]
        _lib = L
    return _lib


def variants() -> dict:
    """variant -> (tile columns, tile rows, slots of the pass table, slots of the count table)"""
    L = lib()
    out = {}
    for v in range(L.th_variants()):
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert L.th_variant(v, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == 0
        out[v] = (a.value, b.value, c.value, d.value)
    return out


def batch() -> int:
    """G: the sweeps of one batch (SPILL_BATCH)."""
    return int(lib().th_batch())


class HostMap:
    """The top records of one snapshot's columns on the host (held by this library's copy of drainage_host)."""

    def __init__(self, s: Snapshot):
        self.L = lib()
        self.dimx, self.dimy = int(s.dimx), int(s.dimy)
        arr = [np.ascontiguousarray(a, dt) for a, dt in ((s.count, np.uint32), (s.type, np.uint32), (s.size, np.float64), (s.floor, np.float64))]
        self.h = self.L.dh_create(self.dimx, self.dimy, *[capi.ptr(a) for a in arr])

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dh_destroy(self.h); self.h = None


def through_many(maps, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes: bool = True):
    """The kernels' bodies over `maps` in one go (the ensemble path) -> ([(records, planes dict or None, nbasins) per map],
    (level sweeps, hop sweeps, batches)); cap None: two calls, a count and the fetch. order: bit 0 the workgroups, bit 1 the lanes,
    last to first."""
    L = lib()
    n = len(maps)
    hs = (C.c_void_p * n)(*[m.h for m in maps])
    nb = np.zeros(n, np.uint32)
    sw = np.zeros(3, np.uint32)
    if cap is None:
        assert L.th_through(hs, n, variant, lanes, order, 0, None, C.sizeof(capi.Through), capi.ptr(nb), None, None, capi.ptr(sw)) == 0
        cap = int(nb.max()) if n else 0
    out = (capi.Through * max(1, n * cap))()
    words = sum(m.dimx * m.dimy for m in maps)
    area = np.zeros(words, np.uint32) if planes else None
    outlets = np.zeros(words, np.uint32) if planes else None
    assert L.th_through(hs, n, variant, lanes, order, cap, out, C.sizeof(capi.Through), capi.ptr(nb), capi.ptr(area), capi.ptr(outlets), capi.ptr(sw)) == 0
    res, at = [], 0
    for i, m in enumerate(maps):
        k = min(cap, int(nb[i]))
        cells = m.dimx * m.dimy
        pl = {"through_area": area[at:at + cells].reshape(m.dimx, m.dimy).copy(), "outlets": outlets[at:at + cells].reshape(m.dimx, m.dimy).copy()} if planes else None
        res.append(([out[i * cap + r].as_dict() for r in range(k)], pl, int(nb[i])))
        at += cells
    return res, tuple(int(v) for v in sw)


def through(s: Snapshot, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes: bool = True):
    """((records, planes, nbasins), (level sweeps, hop sweeps, batches)) of one snapshot."""
    res, sweeps = through_many([HostMap(s)], variant, lanes, order, cap, planes)
    return res[0], sweeps
