"""ctypes wrapper of tests/prox_host (soil_prox.h compiled for the host -- TEST INFRASTRUCTURE ONLY). The build rule, the maps and the
check-program runner are those of analysis_host_lib; the entry takes a list in front of its records and bins behind its counts, so
it is bound here."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from analysis_host_lib import Analysis, Drainage, run_check   # noqa: F401  (the tests take the runner from here)
from soilmachine_amd import capi

u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
POISON = 0xDEADBEEF


class Proximity(Analysis):
    name, entry, record = "prox", "ph_proximity", capi.Proximity
    headers = ("soil_drain.h", "soil_prox.h")
    includes = (Drainage,)
    planes = {"nearest": np.uint32, "group": np.uint32, "dist2": np.uint32}

    def lib(self):
        """Analysis.lib's build rule and maps; this entry's own shape bound instead of the common one."""
        if self._lib is None:
            so, src = os.path.join(self.HERE, f"lib{self.name}_host.so"), self.sources()
            if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in src):
                subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src[0]])
            L = C.CDLL(so)
            L.dh_create.restype, L.dh_create.argtypes = vp, [C.c_int, C.c_int, vp, vp, vp, vp]
            L.dh_destroy.restype, L.dh_destroy.argtypes = None, [vp]
            L.dh_variant.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3
            L.ph_proximity.argtypes = [vp, u32, C.c_int, u32, C.c_int, vp, u32, vp, u64, u32, vp, vp, u32, u32, vp, vp, vp, u32]
            L.ph_bands.restype = u32
            self._lib = L
        return self._lib

    def run_many(self, maps, cells=None, bins: int = 0, bin_width: int = 1, variant: int = 0, lanes: int = 256, order: int = 0, planes=None, cap: int | None = None, bands: int | None = None):
        """One (records, planes, nrecords) per map: the kernels' bodies over `maps` in one go (the ensemble path) with ONE list
        (None: the wet cells). order: bit 0 the workgroups, bit 1 the lanes of the steps without a barrier, last to first. planes:
        the names asked for (default all). cap None: the list's length, or two calls in WATER mode, a count and the fetch. The
        record and row tables are poisoned first: whatever the call does not write shows. bands: the bands of columns the envelopes are built in
        (None: the library's, PROX_BANDS)."""
        L = self.lib()
        nm = len(maps)
        bands = int(L.ph_bands()) if bands is None else int(bands)
        cl, n = capi.proximity_cells(cells, maps[0].dimy)
        hs = (vp * max(1, nm))(*[m.h for m in maps])
        counts = np.zeros(max(1, nm), np.uint32)
        if cap is None:
            cap = n
            if cl is None:
                assert L.ph_proximity(hs, nm, variant, lanes, order, None, 0, None, C.sizeof(capi.Proximity), 0, capi.ptr(counts), None, 0, 1, None, None, None, bands) == 0
                cap = int(counts[:nm].max())
        size = C.sizeof(capi.Proximity)
        out = (capi.Proximity * max(1, nm * cap))()
        C.memset(out, 0xEE, C.sizeof(out))
        words = sum(m.dimx * m.dimy for m in maps)
        want = self.PLANES if planes is None else planes
        pl = {k: np.full(words, POISON, np.uint32) for k in want}
        hist = np.full((max(1, nm), cap, bins), POISON, np.uint32) if bins else None
        rc = L.ph_proximity(hs, nm, variant, lanes, order, capi.ptr(cl), n, out if cap else None, size, cap, capi.ptr(counts), capi.ptr(hist), bins, bin_width,
                            *[capi.ptr(pl.get(k)) for k in self.PLANES], bands)
        assert rc == 0, rc
        res, at = [], 0
        for i, m in enumerate(maps):
            c = m.dimx * m.dimy
            k = min(cap, int(counts[i]))
            recs = [out[i * cap + r].as_dict() for r in range(k)]
            for r in range(k, cap):                       # the records a map does not have stay as they were
                assert out[i * cap + r].site == 0xEEEEEEEE
            for r, rec in enumerate(recs if bins else ()):
                rec["buffers"] = hist[i, r].copy()
            if bins:
                assert (hist[i, k:] == POISON).all()
            res.append((recs, {p: v[at:at + c].reshape(m.dimx, m.dimy).copy() for p, v in pl.items()}, int(counts[i])))
            at += c
        return res

    def run(self, s, cells=None, **kw):
        """(records, planes, nrecords) of one snapshot."""
        return self.run_many([self.HostMap(s)], cells, **kw)[0]


proximity = Proximity()
