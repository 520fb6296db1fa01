"""ctypes wrapper of tests/budget_host (soil_budget.h compiled for the host behind the drainage chain of tests/drainage_host -- TEST
INFRASTRUCTURE ONLY). The build rule, the variants and the check-program runner are those of analysis_host_lib; a map here holds full
columns, laid out as tests/strata_host lays them out."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from analysis_host_lib import Analysis, Drainage, build_check, run_check   # noqa: F401  (the tests take the two runners from here)
from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p


class BadChain(Exception):
    """-5: .cell is the lowest bad cell, .map 0 for the base and 1 + i for member i"""

    def __init__(self, cell: int, which: int):
        super().__init__(f"corrupt chain: map {which}, cell {cell}")
        self.cell, self.map = cell, which


class Budget(Analysis):
    name, entry, headers = "budget", "bh_budget", ("soil_drain.h", "soil_strata.h", "soil_budget.h")
    includes, maps, shapes = (Drainage,), "bh", ("bh", 3, 3)
    planes = {"dground": np.float64, "dheight": np.float64, "dsolid": np.int64, "dwater": np.int64}

    def lib(self):
        """Analysis.lib's build rule; a map of full columns and this entry's own shape bound instead of the common ones."""
        if self._lib is None:
            self._lib = self._build()
        return self._lib

    def _build(self):
        so, src = os.path.join(self.HERE, f"lib{self.name}_host.so"), self.sources()
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in src):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src[0]])
        L = C.CDLL(so)
        L.bh_create.restype, L.bh_create.argtypes = vp, [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, u32]
        L.bh_destroy.restype, L.bh_destroy.argtypes = None, [vp]
        L.bh_pool_size.restype, L.bh_pool_size.argtypes = u64, [vp]
        L.bh_prev.restype, L.bh_prev.argtypes = u32, [vp, C.c_int, u64, C.c_int, u32]
        L.bh_variant.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3
        L.bh_budget.argtypes = [vp, vp, u32, C.c_int, u32, C.c_int, u32, vp, u64, C.POINTER(u32), vp, u64, u32, vp, vp, vp, vp, vp]
        assert L.bh_rec_bytes(0) == C.sizeof(capi.BudgetBasin) and L.bh_rec_bytes(1) == C.sizeof(capi.BudgetSoil)
        return L


budget = Budget()


class HostMap:
    """One snapshot's columns as cell records and a pool on the host."""

    def __init__(self, s: Snapshot, scramble: bool = True, slack: int = 5):
        self.L = budget.lib()
        self.dimx, self.dimy = int(s.dimx), int(s.dimy)
        arr = [np.ascontiguousarray(a, dt) for a, dt in ((s.count, np.uint32), (s.type, np.uint32), (s.size, np.float64), (s.floor, np.float64), (s.sat, np.float64))]
        self.h = self.L.bh_create(self.dimx, self.dimy, *[capi.ptr(a) for a in arr], int(scramble), slack)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.bh_destroy(self.h); self.h = None

    @property
    def pool_size(self) -> int:
        return int(self.L.bh_pool_size(self.h))

    def prev(self, at: int, pool: bool = False, value: int | None = None) -> int:
        """the prev word of cell `at`'s top record (or of pool record `at`); `value`: overwrite it"""
        return int(self.L.bh_prev(self.h, int(pool), at, int(value is not None), int(value or 0)))


def rc_of(base, maps, variant=0, lanes=256, order=0, cap=0, ntypes=None, struct_size=None, soil_struct_size=None) -> int:
    """The return code of a call that asks for the count (and a soil table where ntypes is given) only."""
    L = budget.lib()
    hs = (vp * max(1, len(maps)))(*[m.h for m in maps])
    n = u32()
    out = (capi.BudgetBasin * max(1, len(maps) * cap))() if cap else None
    soils = (capi.BudgetSoil * max(1, len(maps) * max(ntypes, 0)))() if ntypes is not None else None
    return L.bh_budget(base.h if base else None, hs, len(maps), variant, lanes, order, cap, out, C.sizeof(capi.BudgetBasin) if struct_size is None else struct_size,
                       C.byref(n), soils, C.sizeof(capi.BudgetSoil) if soil_struct_size is None else soil_struct_size, ntypes or 0, None, None, None, None, None)


def run_many(base: HostMap, maps, ntypes: int | None = 64, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=(), into=None):
    """The kernels' bodies over `maps` against `base` in one go -> ([(basins, soils, planes dict) per map], nbasins). ntypes None: no
    soil table. cap None: two calls, a count and the fetch, as the Python binding does. planes: the names asked for (one map only).
    into: (out, soils, planes dict) to write to instead of fresh arrays. order: bit 0 the workgroups, bit 1 the lanes, last to first.
    Raises BadChain."""
    L = budget.lib()
    nm = len(maps)
    hs = (vp * max(1, nm))(*[m.h for m in maps])
    n, info = u32(), np.zeros(2, np.uint64)
    size_b, size_s = C.sizeof(capi.BudgetBasin), C.sizeof(capi.BudgetSoil)

    def call(cap, out, soils, pl):
        rc = L.bh_budget(base.h, hs, nm, variant, lanes, order, cap, out, size_b, C.byref(n), soils, size_s, ntypes or 0, *[capi.ptr(pl.get(k)) for k in budget.PLANES],
                         capi.ptr(info))
        if rc == -5:
            raise BadChain(int(info[1]), int(info[0]))
        assert rc == 0, rc

    if cap is None:
        call(0, None, None, {})
        cap = int(n.value)
    if into is None:
        out = (capi.BudgetBasin * max(1, nm * cap))()
        soils = (capi.BudgetSoil * max(1, nm * ntypes))() if ntypes else None
        pl = {k: np.zeros(base.dimx * base.dimy, budget.planes[k]) for k in planes}
    else:
        out, soils, pl = into
    call(cap, out, soils, pl)
    k = min(cap, int(n.value))
    res = [([out[i * cap + r].as_dict() for r in range(k)], [soils[i * ntypes + t].as_dict() for t in range(ntypes)] if ntypes else None,
            {p: v.reshape(base.dimx, base.dimy) for p, v in pl.items()}) for i in range(nm)]
    return res, int(n.value)


def run(base: HostMap, now: HostMap, ntypes: int | None = 64, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=tuple(budget.planes)):
    """((basins, soils, planes), nbasins) of one pair."""
    res, n = run_many(base, [now], ntypes, variant, lanes, order, cap, planes)
    return res[0], n
