"""ctypes wrapper of tests/horizons_host (soil_horizon.h compiled for the host -- TEST INFRASTRUCTURE ONLY). The build rule, the maps
and the check-program runner are those of analysis_host_lib; the entry takes a mask, a reach and suns and has no cap and no count, and
the variants are tile sides (fine, coarse), so both are bound here."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from analysis_host_lib import Analysis, Drainage, build_check, run_check, write_columns   # noqa: F401  (the tests take the runners from here)
from soilmachine_amd import capi

u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p


class Horizons(Analysis):
    name, entry, record = "horizons", "hz_horizons", capi.Horizon
    headers = ("soil_drain.h", "soil_horizon.h")
    includes = (Drainage,)
    shapes = ("hz", 2, 2)
    planes = {"slope": np.float64, "step": np.uint32, "sky": np.float64, "open": np.uint32, "lit": np.uint32}
    defines = ()                # (NoTiles: the scan that walks every step)

    def lib(self):
        """Analysis.lib's build rule and maps; this entry's own shape bound instead of the common one."""
        if self._lib is None:
            tag = "".join("_" + d.lower() for d in self.defines)
            so, src = os.path.join(self.HERE, f"lib{self.name}_host{tag}.so"), self.sources()
            if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in src):
                subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", *["-D" + d for d in self.defines], "-o", so, src[0]])
            L = C.CDLL(so)
            L.dh_create.restype, L.dh_create.argtypes = vp, [C.c_int, C.c_int, vp, vp, vp, vp]
            L.dh_destroy.restype, L.dh_destroy.argtypes = None, [vp]
            L.hz_variant.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 2
            L.hz_horizons.argtypes = [vp, u32, C.c_int, u32, C.c_int, u32, u32, vp, u64, vp, u32, vp, vp, vp, vp, vp, vp, vp]
            self._lib = L
        return self._lib

    def run_many(self, maps, mask: int = 0xFFFF, reach: int = 0, suns=(), variant: int = 0, lanes: int = 256, order: int = 0, planes=None, struct_size: int | None = None):
        """One (records with lit_cells, planes, lit_cells, probes) per map: the kernels' bodies over `maps` in one go (the ensemble
        path) with ONE mask, reach and sun list. suns: (d, tangent) pairs. order: bit 0 the workgroups, bit 1 the lanes of the sky
        step, last to first. planes: the names asked for (default all; `lit` only with suns). probes: (rays, tile bounds, heights
        loaded) of the whole call. struct_size: the prefix of each record asked for; the rest stays as the canary 0xEE."""
        L = self.lib()
        nm = len(maps)
        ds = [d for d in range(16) if mask >> d & 1]
        nd, ns = len(ds), len(suns)
        size = C.sizeof(capi.Horizon)
        out = (capi.Horizon * max(1, nm * nd))()
        C.memset(out, 0xEE, C.sizeof(out))
        words = sum(m.dimx * m.dimy for m in maps)
        want = [p for p in (self.PLANES if planes is None else planes) if p != "lit" or ns]
        pl = {k: np.zeros(words * (nd if k in ("slope", "step") else 1), self.planes[k]) for k in want}
        sl = capi.horizon_suns(list(suns)) if ns else None
        counts = np.zeros(max(1, nm * ns), np.uint32)
        probes = np.zeros(3, np.uint64)
        hs = (vp * max(1, nm))(*[m.h for m in maps])
        rc = L.hz_horizons(hs, nm, variant, lanes, order, mask, reach, out, size if struct_size is None else struct_size, sl, ns, capi.ptr(counts) if ns else None,
                           *[capi.ptr(pl.get(k)) for k in self.PLANES], capi.ptr(probes))
        assert rc == 0, rc
        take = size if struct_size is None else min(size, struct_size)
        raw = bytes(out)

        def record(j):      # record j lies at byte j * struct_size: its prefix, the rest left as the canary
            rec = capi.Horizon()
            C.memset(C.byref(rec), 0xEE, size)
            C.memmove(C.byref(rec), raw[j * take:(j + 1) * take], take)
            return rec.as_dict()

        res, at = [], 0
        for i, m in enumerate(maps):
            c = m.dimx * m.dimy
            mine = {}
            for p, v in pl.items():
                mine[p] = (v.reshape(nd, words)[:, at:at + c].reshape(nd, m.dimx, m.dimy) if p in ("slope", "step") else v[at:at + c].reshape(m.dimx, m.dimy)).copy()
            cnt = [int(v) for v in counts[i * ns:(i + 1) * ns]]
            recs = [record(i * nd + j) for j in range(nd)]
            for r in recs:
                r["lit_cells"] = [cnt[k] for k in range(ns) if suns[k][0] == r["direction"]]
            res.append((recs, mine, cnt, tuple(int(v) for v in probes)))
            at += c
        return res

    def run(self, s, mask: int = 0xFFFF, reach: int = 0, suns=(), variant: int = 0, lanes: int = 256, order: int = 0, planes=None):
        """(records, planes, lit_cells, probes) of one snapshot."""
        return self.run_many([self.HostMap(s)], mask, reach, suns, variant, lanes, order, planes)[0]


class HorizonsNoTiles(Horizons):
    """The same bodies with the tile levels switched off: every step of every ray is loaded (the yardstick of the probe counts)."""
    defines = ("SMX_HORIZON_NO_TILES",)


horizons = Horizons()
horizons_no_tiles = HorizonsNoTiles()
