"""ctypes wrapper of tests/dispersal_host (soil_disp.h compiled for the host -- TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dispersal_host")
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libdispersal_host.so")
SRC = [os.path.join(HERE, "dispersal_host.cpp"), os.path.join(os.path.dirname(HERE), "drainage_host", "drainage_host.cpp")] + \
      [os.path.join(ROOT, "soilmachine_amd", "csrc", f) for f in ("soil_core.h", "soil_lakes.h", "soil_drain.h", "soil_disp.h")]
PLANES = ("area", "donors", "receivers")
FLOW_BLOCKS = 1024                     # DISP_FLOW_BLOCKS of soil_disp.h
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
        L.dph_dispersal.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(C.c_uint32)]
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


def dispersal_rc(maps, exponent: int, variant: int = 0, lanes: int = 256, order: int = 0, flow_blocks: int = FLOW_BLOCKS) -> int:
    """The return code of a counting call (no records, no planes)."""
    n = len(maps)
    hs = (C.c_void_p * n)(*[m.h for m in maps])
    ns = np.zeros(max(1, n), np.uint32)
    return lib().dph_dispersal(hs, n, variant, lanes, order, flow_blocks, exponent, 0, None, capi.ptr(ns), None, None, None, None)


def dispersal_many(maps, exponent: int = 1, variant: int = 0, lanes: int = 256, order: int = 0, flow_blocks: int = FLOW_BLOCKS, cap: int | None = None, planes=PLANES):
    """The kernels' bodies over `maps` in one go (the ensemble path) -> one (records, planes, nbasins, rounds) per map; cap None: two
    calls, a count and the fetch, as the Python binding does. order: bit 0 the workgroups, bit 1 the lanes, last to first; bits 2
    and 3 flip those two for the flow launches alone."""
    L = lib()
    n = len(maps)
    hs = (C.c_void_p * n)(*[m.h for m in maps])
    ns = np.zeros(n, np.uint32)
    rounds = C.c_uint32()
    if cap is None:
        assert L.dph_dispersal(hs, n, variant, lanes, order, flow_blocks, exponent, 0, None, capi.ptr(ns), None, None, None, None) == 0
        cap = int(ns.max()) if n else 0
    out = (capi.Dispersal * max(1, n * cap))()
    words = sum(m.dimx * m.dimy for m in maps)
    pl = {k: np.zeros(words, np.uint64 if k == "area" else np.uint32) for k in planes}
    assert L.dph_dispersal(hs, n, variant, lanes, order, flow_blocks, exponent, cap, out, capi.ptr(ns), *[capi.ptr(pl.get(k)) for k in PLANES], C.byref(rounds)) == 0
    res, at = [], 0
    for i, m in enumerate(maps):
        k = min(cap, int(ns[i]))
        cells = m.dimx * m.dimy
        res.append(([out[i * cap + r].as_dict() for r in range(k)], {p: v[at:at + cells].reshape(m.dimx, m.dimy).copy() for p, v in pl.items()}, int(ns[i]), int(rounds.value)))
        at += cells
    return res


def dispersal(s, exponent: int = 1, variant: int = 0, lanes: int = 256, order: int = 0, flow_blocks: int = FLOW_BLOCKS, cap: int | None = None, planes=PLANES):
    """(records, planes, nbasins, rounds) of one snapshot."""
    return dispersal_many([HostMap(s)], exponent, variant, lanes, order, flow_blocks, cap, planes)[0]
