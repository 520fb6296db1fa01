"""ctypes wrapper of tests/catchments_host (soil_catch.h compiled for the host behind the drainage chain of tests/drainage_host -- TEST
INFRASTRUCTURE ONLY). The build rule, the maps, the variants and the check-program runner are those of analysis_host_lib; the entry
takes a list and has no cap and no count, so it is bound here."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from analysis_host_lib import Analysis, Drainage, build_check, run_check, write_columns   # noqa: F401  (the tests take the runners from here)
from soilmachine_amd import capi

u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p


class Catchments(Analysis):
    name, entry, record = "catchments", "ch_catchments", capi.Catchment
    headers = ("soil_drain.h", "soil_streams.h", "soil_hills.h", "soil_catch.h")
    includes = (Drainage,)
    planes = {"gauge": np.uint32, "straight": np.uint32, "diagonal": np.uint32, "drop": np.float64}

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
            L.ch_catchments.argtypes = [vp, u32, C.c_int, u32, C.c_int, vp, u32, vp, u64, vp, u32, C.c_double, vp, vp, vp, vp, C.POINTER(u32)]
            self._lib = L
        return self._lib

    def run_many(self, maps, cells, variant: int = 0, lanes: int = 256, order: int = 0, planes=None, bins: int = 0, bin_height: float = 1.0, struct_size: int | None = None):
        """One (records, planes, hist or None, rounds) per map: the kernels' bodies over `maps` in one go (the ensemble path) with ONE
        list. order: bit 0 the workgroups, bit 1 the lanes, last to first. struct_size: the prefix of each record asked for; the rest
        of every returned record stays as the canary 0xEE."""
        L = self.lib()
        nm = len(maps)
        cl = np.ascontiguousarray(cells, np.uint32)
        n = len(cl)
        size = C.sizeof(capi.Catchment)
        out = (capi.Catchment * max(1, nm * n))()
        C.memset(out, 0xEE, C.sizeof(out))
        hist = np.zeros((nm, n, bins), np.uint32) if bins else None
        words = sum(m.dimx * m.dimy for m in maps)
        want = self.PLANES if planes is None else planes
        pl = {k: np.zeros(words, self.planes[k]) for k in want}
        rounds = u32()
        hs = (vp * max(1, nm))(*[m.h for m in maps])
        rc = L.ch_catchments(hs, nm, variant, lanes, order, capi.ptr(cl), n, out, size if struct_size is None else struct_size, capi.ptr(hist), bins, float(bin_height),
                             *[capi.ptr(pl.get(k)) for k in self.PLANES], C.byref(rounds))
        assert rc == 0, rc
        take = size if struct_size is None else min(size, struct_size)
        raw = bytes(out)

        def record(j):      # record j lies at byte j * struct_size: its prefix, the rest left as the canary
            rec = capi.Catchment()
            C.memset(C.byref(rec), 0xEE, size)
            C.memmove(C.byref(rec), raw[j * take:(j + 1) * take], take)
            return rec.as_dict()

        res, at = [], 0
        for i, m in enumerate(maps):
            c = m.dimx * m.dimy
            res.append(([record(i * n + r) for r in range(n)], {p: v[at:at + c].reshape(m.dimx, m.dimy).copy() for p, v in pl.items()},
                        hist[i].copy() if bins else None, int(rounds.value)))
            at += c
        return res

    def run(self, s, cells, variant: int = 0, lanes: int = 256, order: int = 0, planes=None, bins: int = 0, bin_height: float = 1.0):
        """(records, planes, hist, rounds) of one snapshot."""
        return self.run_many([self.HostMap(s)], cells, variant, lanes, order, planes, bins, bin_height)[0]


catchments = Catchments()
