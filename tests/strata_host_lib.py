"""ctypes wrapper of tests/strata_host (soil_strata.h compiled for the host -- TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strata_host")
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libstrata_host.so")
SRC = [os.path.join(HERE, "strata_host.cpp")] + [os.path.join(ROOT, "soilmachine_amd", "csrc", f) for f in ("soil_core.h", "soil_strata.h")]
_lib = None


class BadChain(Exception):
    """-5: .cell is the lowest bad cell, .member the first member that has one (totals)"""

    def __init__(self, cell: int, member: int = 0):
        super().__init__(f"corrupt chain: member {member}, cell {cell}")
        self.cell, self.member = cell, member


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in SRC):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", LIB, SRC[0]])
        L = C.CDLL(LIB)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.sh_create.restype = vp
        L.sh_create.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, u32]
        L.sh_destroy.argtypes = [vp]; L.sh_destroy.restype = None
        L.sh_pool_size.argtypes = [vp]; L.sh_pool_size.restype = u64
        L.sh_prev.argtypes = [vp, C.c_int, u64, C.c_int, u32]; L.sh_prev.restype = u32
        L.sh_totals.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
        L.sh_thickness.argtypes = [vp, u32, u32, vp, C.c_int32, vp, vp, vp, vp]
        L.sh_cores.argtypes = [vp, u32, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp]
        assert L.sh_rec_bytes() == C.sizeof(capi.SoilTotal)
        _lib = L
    return _lib


class HostMap:
    """One snapshot's columns as cell records and a pool on the host."""

    def __init__(self, s: Snapshot, scramble: bool = True, slack: int = 5):
        self.L = lib()
        self.dimx, self.dimy = int(s.dimx), int(s.dimy)
        arr = [np.ascontiguousarray(a, dt) for a, dt in ((s.count, np.uint32), (s.type, np.uint32), (s.size, np.float64), (s.floor, np.float64), (s.sat, np.float64))]
        self.h = self.L.sh_create(self.dimx, self.dimy, *[capi.ptr(a) for a in arr], int(scramble), slack)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.sh_destroy(self.h); self.h = None

    @property
    def pool_size(self) -> int:
        return int(self.L.sh_pool_size(self.h))

    def prev(self, at: int, pool: bool = False, value: int | None = None) -> int:
        """the prev word of cell `at`'s top record (or of pool record `at`); `value`: overwrite it"""
        return int(self.L.sh_prev(self.h, int(pool), at, int(value is not None), int(value or 0)))


def totals_many(maps, ntypes: int, lanes: int = 64, nblocks: int = 8, start=None, out=None, other=None):
    """-> one (records, other_sections) per map; raises BadChain. start: nm * ntypes capi.SoilTotal the fold begins from."""
    L = lib()
    n = len(maps)
    hs = (C.c_void_p * n)(*[m.h for m in maps])
    out = (capi.SoilTotal * (n * ntypes))() if out is None else out
    other = np.zeros(n, np.uint64) if other is None else other
    info = np.zeros(2, np.uint64)
    rc = L.sh_totals(hs, n, lanes, nblocks, ntypes, out, capi.ptr(other), start, capi.ptr(info))
    if rc == -5:
        raise BadChain(int(info[1]), int(info[0]))
    assert rc == 0, rc
    return [([out[i * ntypes + t].as_dict() for t in range(ntypes)], int(other[i])) for i in range(n)]


def totals(m: HostMap, ntypes: int, lanes: int = 64, nblocks: int = 8, **kw):
    return totals_many([m], ntypes, lanes, nblocks, **kw)[0]


def thickness(m: HostMap, types, lanes: int = 64, nblocks: int = 8, want=(True, True, True), into=None):
    """-> thickness, cover, sections of shape (len(types), ncells), None where not wanted; raises BadChain"""
    L = lib()
    ty = np.ascontiguousarray(types, np.uint32)
    n = m.dimx * m.dimy
    if into is None:
        into = [np.zeros((len(ty), n)) if want[0] else None, np.zeros((len(ty), n)) if want[1] else None, np.zeros((len(ty), n), np.uint32) if want[2] else None]
    bad = C.c_uint64()
    rc = L.sh_thickness(m.h, lanes, nblocks, capi.ptr(ty), len(ty), capi.ptr(into[0]), capi.ptr(into[1]), capi.ptr(into[2]), C.byref(bad))
    if rc == -5:
        raise BadChain(int(bad.value))
    assert rc == 0, rc
    return tuple(into)


def cores(m: HostMap, cells, lanes: int = 64, nblocks: int = 8, cap: int | None = None, into=None):
    """-> (rc, total, count, type, size, floor, sat); cap None: two calls, a count and the fetch; raises BadChain"""
    L = lib()
    cl = np.ascontiguousarray(cells, np.uint32)
    n = len(cl)
    count = np.zeros(n, np.uint32)
    total, bad = C.c_uint64(), C.c_uint64()
    if cap is None:
        rc = L.sh_cores(m.h, lanes, nblocks, capi.ptr(cl), n, capi.ptr(count), 0, C.byref(total), None, None, None, None, C.byref(bad))
        if rc == -5:
            raise BadChain(int(bad.value))
        assert rc in (0, 1), rc
        cap = int(total.value)
    arrs = into or [np.zeros(cap, np.uint32), np.zeros(cap), np.zeros(cap), np.zeros(cap)]
    rc = L.sh_cores(m.h, lanes, nblocks, capi.ptr(cl), n, capi.ptr(count), cap, C.byref(total), *[capi.ptr(a) for a in arrs], C.byref(bad))
    if rc == -5:
        raise BadChain(int(bad.value))
    assert rc in (0, 1), rc
    return (rc, int(total.value), count, *arrs)
